// Driver of tests/test_gpu_host_set_visible.py: Scene::setVisible of the C++ host mirror before and after buildBVH, and the checkpoint
// fingerprint after a change of visibility.  Prints "HIT <stage> <ray> <primitive> <distance as a hex float>" lines.
#include <cstdio>
#include <string>

#include "mcpt_host.hpp"

static void hits(const Scene &scene, const char *stage) {
    const float targets[6][3] = {{185, 82, 169}, {250, 260, 230}, {278, 0, 300}, {278, 548, 280}, {120, 100, 150}, {330, 300, 200}};
    const Vector3f eye(278, 273, -800);
    for (int k = 0; k < 6; ++k) {
        const Vector3f d = (Vector3f(targets[k][0], targets[k][1], targets[k][2]) - eye).normalized();
        const Intersection it = scene.intersect(Ray(eye, d));
        std::printf("HIT %s %d %d %a\n", stage, k, it.primitive, it.happened ? it.distance : -1.0);
    }
    std::fflush(stdout);
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::string models = argv[1];
    Camera cam(40, 30);
    cam.position = Vector3f(278, 273, -800);
    cam.lookAt(Vector3f(278, 273, 0));
    Scene scene(cam);
    Material white(ROUGH_CONDUCTOR), lamp(ROUGH_CONDUCTOR, Vector3f(10, 10, 10));
    white.base_reflectance = Vector3f(0.7f, 0.7f, 0.7f);
    MeshTriangle floor(models + "/cornellbox/floor.obj", &white), box(models + "/cornellbox/shortbox.obj", &white),
        light(models + "/cornellbox/light.obj", &lamp);
    Sphere ball(Vector3f(250, 260, 230), 60, &white);
    scene.Add(&floor);
    scene.Add(&box);
    scene.Add(&light);
    scene.Add(&ball);
    scene.setVisible(1, false);  // the box, before the scene exists: applied by buildBVH
    scene.buildBVH();
    hits(scene, "A");
    scene.setVisible(3, false);  // the ball, on a live scene: applied at the next query
    hits(scene, "B");
    Renderer r;
    r.setSpp(4);
    r.checkpoint_every = 2;
    r.checkpoint_path = argv[2];
    r.path = argv[3];
    r.stop_after = 2;
    r.Render(scene);  // leaves a checkpoint at 2 of 4 spp
    scene.setVisible(1, true);  // the box is back
    r.Render(scene);  // the scene changed: the checkpoint is not resumed, a new one is left at 2 of 4 spp
    r.stop_after = 0;
    r.Render(scene);  // the same scene: resumed
    hits(scene, "C");
    std::printf("HIDDEN %zu\n", scene.hidden().size());
    return 0;
}
