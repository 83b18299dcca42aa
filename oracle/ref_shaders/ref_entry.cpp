// ref_entry.cpp - extern "C" entry points that call the reference's shader functions by name. TEST INFRASTRUCTURE ONLY.
// Compiled together with oracle/_ref/ref_shaders.cpp (the translated text, see translate.py) into
// oracle/_ref/libref_shaders.so. Every entry point works on n vectors at once: arrays are contiguous, floats are float32,
// a vec3 is 3 floats, a Light is 24 floats in the layout of bindless.glsl's struct (== UhGpuLight), a Reservoir is
// (int Y, float W_sum, float W_X, int M) (== UhReservoir).
#include "glsl_compat.h"

namespace ref {

// ---- what the text reads from its surroundings: bindless.glsl's Light and lights buffer, view.glsl's uniform block
// (only the two members the text reads) and luminance()
struct Light {
   vec4 color;
   vec3 pos;
   float range;
   vec3 dir;
   float spot;
   vec3 att;
   float type;
   vec3 intensity;
   float id;
   vec4 pad;
};
static_assert(sizeof(Light) == 96, "Light is 24 floats, scalar layout");
static struct {
   const Light* lights;
} lightsSSBO;
static struct {
   uint num_lights;
   uint max_num_lights_used;
} view;
static inline float luminance(vec3 rgb) { return dot(rgb, vec3(0.2126f, 0.7152f, 0.0722f)); }

#include "ref_shaders.cpp"

static inline vec3 ld3(const float* p) { return vec3(p[0], p[1], p[2]); }
static inline void st3(float* p, vec3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }

extern "C" {

// the lights buffer stays the caller's; it must hold every slot an index can reach (num_lights + 1 where a draw of 1.0 occurs)
void ref_set_lights(const float* lights, uint num_lights, uint max_num_lights_used) {
   lightsSSBO.lights = (const Light*)lights;
   view.num_lights = num_lights;
   view.max_num_lights_used = max_num_lights_used;
}

// ---- random.glsl
void ref_jenkins_hash(int n, const uint* x, uint* out) {
   for (int i = 0; i < n; i++) out[i] = jenkinsHash(x[i]);
}
void ref_init_rng(int n, const uint* pixel_res_frame /*px py resx resy frame*/, uint* out) {
   for (int i = 0; i < n; i++) {
      const uint* a = pixel_res_frame + 5 * i;
      out[i] = initRNG(uvec2(a[0], a[1]), uvec2(a[2], a[3]), a[4]);
   }
}
void ref_random_float(int n, uint* state, float* out) {
   for (int i = 0; i < n; i++) out[i] = randomFloat(state[i]);
}
void ref_random_point_in_unit_sphere(int n, uint* state, float* out) {
   for (int i = 0; i < n; i++) st3(out + 3 * i, randomPointInUnitSphere(state[i]));
}
void ref_random_point_in_unit_disk(int n, uint* state, float* out) {
   for (int i = 0; i < n; i++) {
      vec2 p = randomPointInUnitDisk(state[i]);
      out[2 * i] = p.x, out[2 * i + 1] = p.y;
   }
}

// ---- restir_sampling.glsl
void ref_target_function(int n, const int* light_index, const float* hit_position, float* out) {
   for (int i = 0; i < n; i++) out[i] = target_function(light_index[i], ld3(hit_position + 3 * i));
}
void ref_sample_light_uniform(int n, uint* state, int* index, float* weight) {
   for (int i = 0; i < n; i++) sample_light_uniform(state[i], index[i], weight[i]);
}
void ref_update_reservoir(int n, uint* state, Reservoir* r, const int* Xi, const float* w_i, const int* M) {
   for (int i = 0; i < n; i++) updateReservoir(state[i], r[i], Xi[i], w_i[i], M[i]);
}
void ref_finalize_resampling(int n, Reservoir* r, const float* p_hat) {
   for (int i = 0; i < n; i++) finalize_resampling(r[i], p_hat[i]);
}
void ref_resample(int n, uint* state, const float* hit_position, Reservoir* out) {
   for (int i = 0; i < n; i++) out[i] = resample(state[i], ld3(hit_position + 3 * i));
}

// ---- brdf.glsl
void ref_distribution_ggx(int n, const float* N, const float* H, const float* roughness, float* out) {
   for (int i = 0; i < n; i++) out[i] = DistributionGGX(ld3(N + 3 * i), ld3(H + 3 * i), roughness[i]);
}
void ref_geometry_schlick_ggx(int n, const float* NdotV, const float* roughness, float* out) {
   for (int i = 0; i < n; i++) out[i] = GeometrySchlickGGX(NdotV[i], roughness[i]);
}
void ref_geometry_smith(int n, const float* N, const float* V, const float* L, const float* roughness, float* out) {
   for (int i = 0; i < n; i++) out[i] = GeometrySmith(ld3(N + 3 * i), ld3(V + 3 * i), ld3(L + 3 * i), roughness[i]);
}
void ref_fresnel_schlick(int n, const float* cosTheta, const float* F0, float* out) {
   for (int i = 0; i < n; i++) st3(out + 3 * i, fresnelSchlick(cosTheta[i], ld3(F0 + 3 * i)));
}
void ref_fresnel_schlick_roughness(int n, const float* cosTheta, const float* F0, const float* roughness, float* out) {
   for (int i = 0; i < n; i++) st3(out + 3 * i, fresnelSchlickRoughness(cosTheta[i], ld3(F0 + 3 * i), roughness[i]));
}
void ref_random(int n, const float* co, float* out) {
   for (int i = 0; i < n; i++) out[i] = random(vec2(co[2 * i], co[2 * i + 1]));
}
void ref_hammersley2d(int n, const uint* i_N, float* out) {
   for (int i = 0; i < n; i++) {
      vec2 p = hammersley2d(i_N[2 * i], i_N[2 * i + 1]);
      out[2 * i] = p.x, out[2 * i + 1] = p.y;
   }
}
void ref_importance_sample_ggx(int n, const float* Xi, const float* roughness, const float* normal, float* out) {
   for (int i = 0; i < n; i++) st3(out + 3 * i, importanceSample_GGX(vec2(Xi[2 * i], Xi[2 * i + 1]), roughness[i], ld3(normal + 3 * i)));
}

// ---- pbr_lighting.glsl. pixel = position 3, baseColor 3, normal 3, metallic, roughness (11 floats); F0 and occlusion of
// PixelParams are not read by surfaceShading
void ref_surface_shading(int n, const float* pixel, const float* light, const float* eyePos, const float* lightColorFactor, float* out) {
   for (int i = 0; i < n; i++) {
      const float* p = pixel + 11 * i;
      PixelParams pp;
      pp.position = ld3(p), pp.baseColor = ld3(p + 3), pp.normal = ld3(p + 6);
      pp.F0 = vec3(0.0f), pp.metallic = p[9], pp.roughness = p[10], pp.occlusion = 1.0f;
      st3(out + 3 * i, surfaceShading(pp, ((const Light*)light)[i], ld3(eyePos + 3 * i), lightColorFactor[i]));
   }
}

// ---- atmosphere.glsl
void ref_sphere_intersection(int n, const float* rayStart, const float* rayDir, const float* sphereCenter, const float* sphereRadius, float* out) {
   for (int i = 0; i < n; i++) {
      vec2 t = SphereIntersection(ld3(rayStart + 3 * i), ld3(rayDir + 3 * i), ld3(sphereCenter + 3 * i), sphereRadius[i]);
      out[2 * i] = t.x, out[2 * i + 1] = t.y;
   }
}
void ref_phase_mie(int n, const float* costh, const float* g, float* out) {
   for (int i = 0; i < n; i++) out[i] = PhaseMie(costh[i], g[i]);
}
void ref_integrate_optical_depth(int n, const float* rayStart, const float* rayDir, float* out) {
   for (int i = 0; i < n; i++) st3(out + 3 * i, IntegrateOpticalDepth(ld3(rayStart + 3 * i), ld3(rayDir + 3 * i)));
}
void ref_integrate_scattering(int n, const float* rayStart, const float* rayDir, const float* rayLength, const float* lightDir,
                              const float* lightColor, float* color, float* transmittance) {
   for (int i = 0; i < n; i++) {
      vec3 t;
      st3(color + 3 * i, IntegrateScattering(ld3(rayStart + 3 * i), ld3(rayDir + 3 * i), rayLength[i], ld3(lightDir + 3 * i), ld3(lightColor + 3 * i), t));
      st3(transmittance + 3 * i, t);
   }
}
}
}  // namespace ref
