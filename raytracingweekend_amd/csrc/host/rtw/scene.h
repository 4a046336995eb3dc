// scene.h — scene container + the reference's scenes, and the host render API.
//
// `scene` keeps the accessors of the reference (Scene/scene.h:18-40):
// GetWorld, GetLights, GetCamera, GetRenderType, GetBackgroundType, Add.
// The concrete scenes restate Scene/scene.h:42-250 (light_sample,
// dielectric_scene, random_balls_scene, cornell_box_scene) plus Book 2's
// final scene (not in the reference; see scenes.cpp).
#pragma once
#include <memory>
#include <string>
#include <vector>
#include "camera.h"
#include "hittable_list.h"

enum class RenderType { Shaded, Normal };
enum class BackgroundType { Black, Gradient };

class scene {
public:
    scene() {}
    virtual ~scene() {}

    void Add(std::shared_ptr<hittable> h) { world.objects.push_back(h); }
    const hittable_list& GetWorld() const { return world; }
    std::shared_ptr<hittable_list> GetLights() const { return lights; }
    RenderType GetRenderType() const { return render_type; }
    BackgroundType GetBackgroundType() const { return background_type; }
    camera& GetCamera() { return cam; }
    const camera& GetCamera() const { return cam; }

protected:
    hittable_list world;
    std::shared_ptr<hittable_list> lights = std::make_shared<hittable_list>();
    camera cam;
    RenderType render_type = RenderType::Shaded;
    BackgroundType background_type = BackgroundType::Gradient;
};

class light_sample : public scene {
public:
    explicit light_sample(double aspect);
};
class dielectric_scene : public scene {
public:
    explicit dielectric_scene(double aspect);
};
class random_balls_scene : public scene {
public:
    explicit random_balls_scene(double aspect);
};
class cornell_box_scene : public scene {
public:
    explicit cornell_box_scene(double aspect);
};
class book2_final_scene : public scene {
public:
    explicit book2_final_scene(double aspect);
};
// Test scene for arbitrary nesting (transforms and media inside lists).
class nested_scene : public scene {
public:
    explicit nested_scene(double aspect, bool media = true);
};
// Test scene for group BVHs without media: two transformed lists (spheres,
// boxes) among plain balls; `extra` adds plain spheres for a world BVH.
class grouped_scene : public scene {
public:
    explicit grouped_scene(double aspect, bool extra = false);
};

// Test scenes for the equal-distance rule of hittable_list::hit (scenes.cpp):
// "ties" is made of twins, primitives of identical geometry and different
// material and normal, of every class and in every walk; "ties_axis" holds
// stations where a sphere and a rect touch on an axis-parallel ray.
class ties_scene : public scene {
public:
    explicit ties_scene(double aspect);
};
class ties_axis_scene : public scene {
public:
    explicit ties_axis_scene(double aspect);
};

// Test scene for image textures (not in the reference, whose scenes use
// none): two images computed in code on every primitive kind (scenes.cpp).
// `first`, when given, replaces the first image (nx * ny RGB texels).
class textured_scene : public scene {
public:
    explicit textured_scene(double aspect, std::shared_ptr<image_texture::byte_array> first = nullptr, int nx = 0,
                            int ny = 0);
    // the scene's own images: 0 = 7 x 5, 1 = 4 x 3
    static std::shared_ptr<image_texture::byte_array> test_image(int which, int& nx, int& ny);
};

// Test scenes for the converged fp32-vs-fp64 comparison
// (tests/test_gpu_fp32_probes.py), one shading feature each under bounded
// radiance: `kind` is one of "rect_light", "sphere_light",
// "far_sphere_light", "default_light", "glass", "metal", "medium", "motion",
// "textures" (scenes.cpp says what each holds).  Any other kind leaves the
// scene empty; make_builtin_scene refuses it.
class probe_scene : public scene {
public:
    probe_scene(double aspect, const std::string& kind);
    static bool has_kind(const std::string& kind);
};

// Builds a scene by name ("cornell_box", "random_balls", "dielectric",
// "light_sample", "book2_final", "nested", "nested_plain", "textured",
// "grouped", "grouped_world", "ties", "ties_axis", and the test scenes
// "probe_<kind>" of probe_scene);
// nullptr for an unknown name.
std::unique_ptr<scene> make_builtin_scene(const std::string& name, double aspect);

// Flatten the hittable graph of `sc` into a library-owned rtw_scene_desc
// (free with rtw_scene_desc_free).  Returns 0 or a negative rtw_status and
// sets rtw_last_error().  use_bvh: build device BVHs (world, and groups with
// more than a handful of primitives).
int rtw_flatten_scene(const scene& sc, int use_bvh, rtw_scene_desc** out);
