// mcpt_host.hpp -- C++ host side above the C ABI (include/mcpt.h).
//
// One header for the whole host mirror: small float vectors, Material, the scene objects (MeshTriangle, Sphere), Camera,
// Scene and Renderer.  Class and member names follow the reference's public interface (Renderer::Render / setSpp / path,
// Scene::Add / setRrRate / setDirectLightSample / enableShadow / loadEnvMap / buildBVH / intersect / castRay,
// MeshTriangle(filename, material, translation, zoom), Sphere(center, radius, material), Camera::lookAt) so that code
// written against the reference compiles against this header; everything that is hot runs in libmcpt_hip.so.
#pragma once
#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mcpt.h"

// ============================================================================ vectors
// Minimal float vectors for the host side (the reference uses Eigen's Vector3f/Vector2f/Matrix3f for the same job).
// Only what scene assembly needs: storage, +, -, scalar *, dot/cross/normalized with Eigen's evaluation order.

struct Vector2f {
    float v[2] = {0.f, 0.f};
    Vector2f() = default;
    Vector2f(float x, float y) : v{x, y} {}
    float x() const { return v[0]; }
    float y() const { return v[1]; }
    float operator[](int i) const { return v[i]; }
};

struct Vector3f {
    float v[3] = {0.f, 0.f, 0.f};
    Vector3f() = default;
    Vector3f(float x, float y, float z) : v{x, y, z} {}
    static Vector3f Zero() { return Vector3f(0.f, 0.f, 0.f); }
    float x() const { return v[0]; }
    float y() const { return v[1]; }
    float z() const { return v[2]; }
    float operator[](int i) const { return v[i]; }
    float &operator[](int i) { return v[i]; }
    const float *data() const { return v; }
    Vector3f operator+(const Vector3f &o) const { return {v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]}; }
    Vector3f operator-(const Vector3f &o) const { return {v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]}; }
    Vector3f operator*(float s) const { return {v[0] * s, v[1] * s, v[2] * s}; }
    float dot(const Vector3f &o) const { return v[0] * o.v[0] + (v[1] * o.v[1] + v[2] * o.v[2]); }
    Vector3f cross(const Vector3f &o) const {
        return {v[1] * o.v[2] - v[2] * o.v[1], v[2] * o.v[0] - v[0] * o.v[2], v[0] * o.v[1] - v[1] * o.v[0]};
    }
    float norm() const { return std::sqrt(dot(*this)); }
    Vector3f normalized() const {
        const float z = dot(*this);
        if (z > 0.f) {
            const float s = std::sqrt(z);
            return {v[0] / s, v[1] / s, v[2] / s};
        }
        return *this;
    }
};
inline Vector3f operator*(float s, const Vector3f &a) { return a * s; }

struct Matrix3f {  // row-major storage, column accessors as the reference uses them (Camera.hpp:21-23)
    float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    static Matrix3f Identity() { return Matrix3f(); }
    void setCol(int j, const Vector3f &c) {
        for (int i = 0; i < 3; ++i) m[3 * i + j] = c[i];
    }
    float operator()(int i, int j) const { return m[3 * i + j]; }
};

// ============================================================================ material

// Host-side Material: the fields and constructor defaults of the reference's Material (src/Material.hpp:157-167,245-257).
// The BSDF itself (sample/eval/pdf/fresnel) runs on the GPU (csrc/mcpt_device.h); the host only describes materials.

enum MaterialType { SMOOTH_CONDUCTOR, ROUGH_CONDUCTOR, SMOOTH_DIELECTRIC, ROUGH_DIELECTRIC };  // Material.hpp:13-18

class Material {
  public:
    MaterialType m_type;
    Vector3f m_emission;
    float iorA, iorB;
    bool textured = false;  // the reference leaves this uninitialised (Material.hpp:164); false is what its renders show
    bool isDirac;
    float roughness;
    Vector3f base_reflectance;

    explicit Material(MaterialType t = ROUGH_CONDUCTOR, Vector3f e = Vector3f(0, 0, 0)) {
        m_type = t;
        m_emission = e;
        isDirac = (t == SMOOTH_CONDUCTOR || t == SMOOTH_DIELECTRIC);
        iorA = 1.74;
        iorB = 0.1f;
        roughness = (t == ROUGH_DIELECTRIC) ? 0.2f : 1.f;
        base_reflectance = Vector3f(0, 0, 0);
    }
    MaterialType getType() const { return m_type; }
    Vector3f getEmission() const { return m_emission; }
    bool hasEmission() const { return m_emission.norm() > 1e-4f; }  // Material.hpp:262
};

// ============================================================================ scene objects

// Host-side scene objects: MeshTriangle and Sphere keep the reference's constructors (src/Triangle.hpp:83-86,
// src/Sphere.hpp:20-21); intersection, bounds and sampling live in the GPU library.


class Object {
  public:
    virtual ~Object() {}
    virtual bool hasEmit() const = 0;
    virtual float getArea() const = 0;
};

struct Triangle {  // src/Triangle.hpp:41-56: world-space vertices + texture coordinates
    Vector3f v0, v1, v2;
    Vector2f t0, t1, t2;
    float area() const { return (v1 - v0).cross(v2 - v0).norm() * 0.5f; }
};

// Per-face vertex stream of the first mesh of an OBJ file, as the reference's loader produces it.
bool load_obj_vertex_stream(const std::string &path, std::vector<Vector3f> &positions, std::vector<Vector2f> &texcoords);

class MeshTriangle : public Object {
  public:
    // Triangle.hpp:83-135: the loader's vertex stream is grouped by threes (the index buffer is ignored, so quads are
    // not triangulated); v = zoom * vert + translation; texture coordinates are copied only for textured materials.
    MeshTriangle(const std::string &filename, Material *mt = new Material(), const Vector3f &translation = Vector3f::Zero(),
                 float zoom = 1.0f);
    bool hasEmit() const override { return m->hasEmission(); }
    float getArea() const override { return area; }
    std::vector<Triangle> triangles;
    float area = 0.f;
    Material *m;
    bool loaded = false;
};

class Sphere : public Object {
  public:
    Vector3f center;
    float radius;
    Material *m;
    Sphere(const Vector3f &c, const float &r, Material *mt = new Material()) : center(c), radius(r), m(mt) {}
    bool hasEmit() const override { return m->hasEmission(); }
    float getArea() const override { return 4 * 3.141592653589793f * radius * radius; }
};

// ============================================================================ camera

// src/Camera.hpp:6-26 restated.

class Camera {
    Matrix3f orientation = Matrix3f::Identity();

  public:
    int width = 1280, height = 960;
    float fov = 40;
    bool useDOF = false;
    float focal_distance = 100;
    float aperture_radius = 5.0f;
    Camera(int w = 1280, int h = 960) : width(w), height(h) {}
    Vector3f position = {0, 0, 0};
    void lookAt(const Vector3f &target, const Vector3f &up = {0, 1, 0}) {
        const Vector3f forward = (target - position).normalized();
        const Vector3f left = up.cross(forward).normalized();
        const Vector3f new_up = forward.cross(left).normalized();
        orientation.setCol(0, left);
        orientation.setCol(1, new_up);
        orientation.setCol(2, forward);
    }
    Matrix3f getOrientation() const { return orientation; }
};

// ============================================================================ scene

// Host-side Scene: the public surface of the reference's Scene (src/Scene.hpp:24-152) over the C ABI.
//   Add / setRrRate / setDirectLightSample / enableShadow / loadEnvMap / backgroundColor / camera / buildBVH
// keep their names and meaning; buildBVH() flattens the objects and uploads them to the GPU (mcpt_scene_create);
// intersect() and castRay() forward to mcpt_intersect / mcpt_cast_rays.


enum WaveLenType { RED, GREEN, BLUE };  // src/WaveLen.hpp:5

struct Ray {  // src/Ray.hpp:6-19 (the inverse direction is computed on the device)
    Vector3f origin, direction;
    Ray(const Vector3f &o, const Vector3f &d) : origin(o), direction(d) {}
};

struct Intersection {  // the parts of src/Intersection.hpp the C ABI reports
    bool happened = false;
    double distance = 1.7976931348623157e308;
    int primitive = -1;
};

class Scene {
    float rrRate = 0.7f;  // Scene.hpp:25
    bool enable_shadow = true;
    int n_dir_sample = 4;  // Scene.hpp:28 (conf.json's directLightSample is never applied by the reference's main)

  public:
    Camera camera;
    Vector3f backgroundColor = Vector3f(0, 0, 0);
    bool useEnvMap = false;
    unsigned envWidth = 0, envHeight = 0;
    std::vector<float> envPixels;  // envWidth*envHeight*3 floats in [0,1]

    explicit Scene(Camera cam) : camera(cam) {}
    ~Scene();
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;

    void loadEnvMap(const std::string &path);  // Scene.hpp:39-57: on failure prints the error and keeps the colour
    void Add(Object *object) {                 // Scene.hpp:104-109
        objects.push_back(object);
        if (object->hasEmit()) lightsObjects.push_back(object);
    }
    void setRrRate(float rr) { rrRate = rr < 0.99f ? rr : 0.99f; }  // Scene.hpp:110-113
    void setDirectLightSample(int x) { n_dir_sample = x; }
    void enableShadow(bool shadow) { enable_shadow = shadow; }
    const std::vector<Object *> &get_objects() const { return objects; }

    void buildBVH();  // Scene.cpp:14-17
    Intersection intersect(const Ray &ray) const;                                // Scene.cpp:19-21
    float castRay(const Ray &ray, int depth, const WaveLenType &wavelen) const;  // Scene.cpp:85-184 (depth must be 0)

    // Moves an object of a live scene: m is a row-major 3x4 matrix applied to the object's geometry AS IT WAS ADDED (transforms are
    // absolute, mcpt_scene_update).  It takes effect at the next buildBVH(), or, when the scene is already built, at the next render,
    // intersect or castRay (mcpt_scene_update / mcpt_group_update: the tree is rebuilt, the handle and its workspaces stay).
    void setTransform(Object *object, const float m[12]);
    // the transforms set so far, in Scene::Add order (object = index into `objects`); objects that are not in the scene are left out
    std::vector<mcpt_object_transform> transforms() const;

    // Hides or shows an object (index into `objects`, Scene::Add order; every object is visible until hidden).  A hidden object keeps its
    // geometry, transform and material and stays out of the tree and the light tables (mcpt_scene_set_visibility: primitive ids do not
    // change).  Like setTransform it takes effect at the next buildBVH(), or, when the scene is already built, at the next render,
    // intersect or castRay (mcpt_scene_set_visibility / mcpt_group_set_visibility).  An index outside the scene is ignored with a message.
    void setVisible(int object, bool visible);
    // the hidden objects, ascending
    std::vector<int32_t> hidden() const;

    // Relights a live scene (mcpt_scene_set_materials / mcpt_scene_set_environment, or their group forms after setDevices).
    // setMaterial gives the object's material the values of `m`: the scene's material table is fixed once built, so a material the scene
    // does not hold cannot be added; the object's own entry is edited, which is refused (false, with a message) when another object
    // shares that Material, or when the object was pointed at another Material after buildBVH().  Before buildBVH() it only changes
    // the Material the object points to.  setBackground replaces the colour
    // and the environment map (env_pixels: env_w * env_h * 3 floats in [0,1], or nullptr with 0, 0 for the constant colour).  On a
    // built scene both take effect at once and return false, with the library's message on stderr, when the library refuses.
    bool setMaterial(Object *object, const Material &m);
    bool setBackground(const Vector3f &color, unsigned env_w = 0, unsigned env_h = 0, const float *env_pixels = nullptr);

    // used by Renderer
    mcpt_scene *handle() const {  // (with several GPUs: the replica on the first one)
        applyTransforms();
        applyVisibility();
        return group ? mcpt_group_scene(group, 0) : gpu;
    }
    // More than one entry: the frame is rendered by all listed GPUs (mcpt_group_*: tile partition + RCCL merge inside the
    // library; main() stays single-threaded).  Call before buildBVH.  {0, 0} rehearses the schedule on one GPU.
    void setDevices(const std::vector<int> &d) { devices = d; }
    mcpt_group *groupHandle() const {
        applyTransforms();
        applyVisibility();
        return group;
    }
    mcpt_params params(int spp) const;
    mcpt_camera cameraDesc() const;
    // flat description (also used by the tests to compare with the Python assembly)
    void flatten(std::vector<mcpt_triangle> &tris, std::vector<mcpt_material> &mats, std::vector<mcpt_object> &objs) const;

    std::vector<Object *> objects;
    std::vector<Object *> lightsObjects;

  private:
    mcpt_scene *gpu = nullptr;
    mcpt_group *group = nullptr;
    std::vector<int> devices;
    void allTransformsPending();
    void applyTransforms() const;  // sends the transforms set since the last call to the live scene
    std::map<const Object *, std::array<float, 12>> objectTransforms;
    mutable std::vector<const Object *> pendingTransforms;
    void applyVisibility() const;  // sends the states set since the last call to the live scene
    std::map<int, bool> objectVisible;         // the objects setVisible was called for
    mutable std::vector<int> pendingVisible;   // those of them the live scene has not heard of yet
    // the Material every object pointed to when buildBVH() numbered the library's material table (flatten(): order of first
    // appearance); setMaterial on a built scene reads the numbering from here, not from pointers that may have changed since
    std::vector<const Material *> builtMaterialOf;
};

// ============================================================================ renderer

// src/Renderer.hpp:14-23 restated: same members, same defaults.


class Renderer {
  public:
    void Render(const Scene &scene);
    void setSpp(int s) { spp = s; }
    std::string path = "./output.png";
    // Pass-wise accumulation with a checkpoint file (the reference's render is all-or-nothing: two hours, Renderer.cpp:36-90).
    // With a checkpoint path the frame is rendered in chunks of `checkpoint_every` spp (mcpt_params.sample_offset / accumulate:
    // the same Philox keys and the same order of additions as one call, so the image is bit-identical), the running frame is
    // written after every chunk, and a later run with the same scene, size, spp and seed continues where the file stops.
    std::string checkpoint_path;
    int checkpoint_every = 64;
    int stop_after = 0;  // test hook: leave after this many spp have been rendered in total (simulates an interruption)
    // Adaptive sampling (mcpt_render_adaptive): spp is then the maximum, adaptive_min the first level (0: 64, or spp when smaller).
    // One GPU; not combined with a checkpoint.
    bool adaptive = false;
    float adaptive_threshold = 0.f;
    int adaptive_min = 0;
    // Denoising (mcpt_render_denoised): the plain frame goes to `path` as without it (bit-identical), the denoised one, through the same
    // tone map, to denoise_path; denoise_aov_spp feature samples per pixel (0: min(4, spp)).  One GPU; not combined with a checkpoint or
    // adaptive sampling.  denoise_specular_depth: mirror / glass bounces the feature samples follow (0: first-hit features).
    std::string denoise_path;
    int denoise_aov_spp = 0;
    int denoise_specular_depth = 0;
    // With adaptive: the adaptive frame through mcpt_render_adaptive_denoised, the denoised frame to this path (denoise_aov_spp and
    // denoise_specular_depth apply; denoise_aov_spp at most the first level).
    std::string adaptive_denoise_path;

  private:
    int spp = 2048;
};
