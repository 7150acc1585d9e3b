// Driver of tests/test_gpu_scene_materials.py: Scene::setMaterial and Scene::setBackground of the C++ host mirror.
//   live   the scene is built, rendered once, edited (mcpt_scene_set_materials / mcpt_scene_set_environment), and rendered to the PNG
//   fresh  the same edits are made before buildBVH: a fresh scene of the edited description
//   group  as live, on two replicas on device 0 (Scene::setDevices)
// The three PNGs must be byte-identical.  Prints "SHARED <0|1>": whether an edit of a material two objects share was accepted, and
// "REPOINTED <0|1>": whether an edit through an object whose Material pointer changed after buildBVH() was.
#include <cstdio>
#include <string>
#include <vector>

#include "mcpt_host.hpp"

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::string models = argv[1], mode = argv[2];
    Camera cam(48, 36);
    cam.position = Vector3f(278, 273, -800);
    cam.lookAt(Vector3f(278, 273, 0));
    Scene scene(cam);
    scene.backgroundColor = Vector3f(0.1f, 0.1f, 0.1f);
    Material white(ROUGH_CONDUCTOR), green(ROUGH_CONDUCTOR), lamp(ROUGH_CONDUCTOR, Vector3f(10, 10, 10)), plastic(ROUGH_DIELECTRIC);
    white.base_reflectance = Vector3f(0.7f, 0.7f, 0.7f);
    green.base_reflectance = Vector3f(0.1f, 0.8f, 0.1f);
    MeshTriangle floor(models + "/cornellbox/floor.obj", &white), tall(models + "/cornellbox/tallbox.obj", &white),
        box(models + "/cornellbox/shortbox.obj", &green), light(models + "/cornellbox/light.obj", &lamp);
    Sphere ball(Vector3f(250, 260, 230), 60, &plastic);
    scene.Add(&floor);
    scene.Add(&tall);
    scene.Add(&box);
    scene.Add(&light);
    scene.Add(&ball);
    if (mode == "group") scene.setDevices({0, 0});

    Material glass(SMOOTH_DIELECTRIC);  // the short box turns into glass: in place
    glass.iorA = 1.5f;
    glass.iorB = 0.01f;
    glass.roughness = 0.01f;
    Material glow(ROUGH_DIELECTRIC, Vector3f(3, 2, 1));  // the ball starts to emit: the host path
    glow.roughness = 0.3f;
    Material dim(ROUGH_CONDUCTOR, Vector3f(4, 4, 5));  // the lamp is dimmed: in place
    std::vector<float> sky((size_t)8 * 4 * 3);
    for (size_t i = 0; i < sky.size(); ++i) sky[i] = (float)((i * 37) % 101) / 100.f;

    Renderer r;
    r.setSpp(4);
    r.path = argv[3];
    if (mode != "fresh") {
        scene.buildBVH();
        r.Render(scene);  // the scene as it was created
    }
    const bool shared = scene.setMaterial(&floor, glass);  // `white` belongs to the floor and the tall box: refused, nothing changes
    bool ok = scene.setMaterial(&box, glass);
    ok = scene.setMaterial(&ball, glow) && ok;
    ok = scene.setMaterial(&light, dim) && ok;
    ok = scene.setBackground(Vector3f(0.2f, 0.3f, 0.4f), 8, 4, sky.data()) && ok;
    box.m = &plastic;  // pointed elsewhere behind the scene's back: a built scene numbered its table with `green`, so the edit is refused
    const bool repointed = scene.setMaterial(&box, dim);  // (before buildBVH the new pointer is simply shared with the ball: refused too)
    box.m = &green;
    if (mode == "fresh") scene.buildBVH();
    r.Render(scene);
    std::printf("SHARED %d\nREPOINTED %d\nEDITS %d\nLIGHTS %zu\n", shared ? 1 : 0, repointed ? 1 : 0, ok ? 1 : 0, scene.lightsObjects.size());
    return 0;
}
