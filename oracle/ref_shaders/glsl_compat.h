// glsl_compat.h - the GLSL types and built-ins that the reference's include files use, in float32 C++.
// TEST INFRASTRUCTURE ONLY. The translated shader text (oracle/_ref/ref_shaders.cpp, made by translate.py and never
// committed) is compiled against this header, so that the reference's own arithmetic, not a reading of it, is what the
// known-answer file tests/golden/ref_shader_kat.npz records.
//
// Rules this header follows:
//  - every operation is one IEEE float32 operation, left to right, never fused (build with -ffp-contract=off);
//  - built-ins whose formula the GLSL specification gives are written by that formula: dot, cross, length = sqrt(dot),
//    distance = length(a - b), reflect = I - 2*dot(N,I)*N, mix = x*(1-a) + y*a, mod = x - y*floor(x/y),
//    fract = x - floor(x), clamp = min(max(x, lo), hi), min/max by comparison;
//  - built-ins whose precision the specification leaves open are evaluated the plainest way: normalize = v / sqrt(dot(v,v))
//    (a division per component), and pow, exp, sin, cos by libm's powf, expf, sinf, cosf. A GPU or the oracle may evaluate
//    these differently (reciprocal-multiply normalize, pow(x, 5) as a product); comparisons through them carry a measured
//    margin, see DESIGN.md section 2;
//  - dot() of two uvec2 converts to float first: GLSL defines dot only for floating-point vectors;
//  - an int operand beside a float (max(0, h), 4 * a, x / count) converts to float, as GLSL's implicit conversion does.
//    The scalar constructors are explicit, so an int never becomes a vector by accident.
#pragma once
#include <cmath>
#include <cstdint>

namespace ref {

typedef uint32_t uint;

struct vec2 {
   float x, y;
   vec2() : x(0), y(0) {}
   explicit vec2(float s) : x(s), y(s) {}
   vec2(float x_, float y_) : x(x_), y(y_) {}
   vec2 xy() const { return *this; }
};
struct vec3 {
   float x, y, z;
   vec3() : x(0), y(0), z(0) {}
   explicit vec3(float s) : x(s), y(s), z(s) {}
   vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
   vec2 xy() const { return vec2(x, y); }
   vec2 xz() const { return vec2(x, z); }
   vec3 rgb() const { return *this; }
};
struct vec4 {
   float x, y, z, w;
   vec4() : x(0), y(0), z(0), w(0) {}
   vec4(float x_, float y_, float z_, float w_) : x(x_), y(y_), z(z_), w(w_) {}
   vec3 rgb() const { return vec3(x, y, z); }
};
struct uvec2 {
   uint x, y;
   uvec2() : x(0), y(0) {}
   uvec2(uint x_, uint y_) : x(x_), y(y_) {}
};

// scalars ----------------------------------------------------------------------------------------
static inline float min(float a, float b) { return b < a ? b : a; }
static inline float max(float a, float b) { return a < b ? b : a; }
static inline uint min(uint a, uint b) { return b < a ? b : a; }
static inline uint max(uint a, uint b) { return a < b ? b : a; }
static inline float clamp(float x, float lo, float hi) { return min(max(x, lo), hi); }
static inline float abs(float x) { return std::fabs(x); }
static inline float sqrt(float x) { return std::sqrt(x); }
static inline float floor(float x) { return std::floor(x); }
static inline float fract(float x) { return x - std::floor(x); }
static inline float mod(float x, float y) { return x - y * std::floor(x / y); }
static inline float pow(float x, float y) { return powf(x, y); }
static inline float exp(float x) { return expf(x); }
static inline float sin(float x) { return sinf(x); }
static inline float cos(float x) { return cosf(x); }

// vec2 -------------------------------------------------------------------------------------------
static inline vec2 operator+(vec2 a, vec2 b) { return vec2(a.x + b.x, a.y + b.y); }
static inline vec2 operator-(vec2 a, vec2 b) { return vec2(a.x - b.x, a.y - b.y); }
static inline vec2 operator-(vec2 a, float s) { return vec2(a.x - s, a.y - s); }
static inline vec2 operator*(vec2 a, float s) { return vec2(a.x * s, a.y * s); }
static inline vec2 operator*(float s, vec2 a) { return vec2(s * a.x, s * a.y); }
static inline vec2 operator/(vec2 a, float s) { return vec2(a.x / s, a.y / s); }
static inline float dot(vec2 a, vec2 b) { return a.x * b.x + a.y * b.y; }
static inline float dot(uvec2 a, uvec2 b) { return dot(vec2((float)a.x, (float)a.y), vec2((float)b.x, (float)b.y)); }

// vec3 -------------------------------------------------------------------------------------------
static inline vec3 operator-(vec3 a) { return vec3(-a.x, -a.y, -a.z); }
static inline vec3 operator+(vec3 a, vec3 b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline vec3 operator-(vec3 a, vec3 b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline vec3 operator*(vec3 a, vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline vec3 operator/(vec3 a, vec3 b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
static inline vec3 operator+(vec3 a, float s) { return vec3(a.x + s, a.y + s, a.z + s); }
static inline vec3 operator+(float s, vec3 a) { return vec3(s + a.x, s + a.y, s + a.z); }
static inline vec3 operator-(vec3 a, float s) { return vec3(a.x - s, a.y - s, a.z - s); }
static inline vec3 operator-(float s, vec3 a) { return vec3(s - a.x, s - a.y, s - a.z); }
static inline vec3 operator*(vec3 a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
static inline vec3 operator*(float s, vec3 a) { return vec3(s * a.x, s * a.y, s * a.z); }
static inline vec3 operator/(vec3 a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
static inline vec3& operator+=(vec3& a, vec3 b) { return a = a + b; }
static inline vec3& operator-=(vec3& a, vec3 b) { return a = a - b; }
static inline vec3& operator*=(vec3& a, float s) { return a = a * s; }
static inline float dot(vec3 a, vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static inline vec3 cross(vec3 a, vec3 b) { return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
static inline float length(vec3 a) { return std::sqrt(dot(a, a)); }
static inline float distance(vec3 a, vec3 b) { return length(a - b); }
static inline vec3 normalize(vec3 a) { return a / std::sqrt(dot(a, a)); }
static inline vec3 reflect(vec3 I, vec3 N) { return I - 2.0f * dot(N, I) * N; }
static inline vec3 mix(vec3 x, vec3 y, float a) { return x * (1.0f - a) + y * a; }
static inline vec3 max(vec3 a, vec3 b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
static inline vec3 exp(vec3 a) { return vec3(expf(a.x), expf(a.y), expf(a.z)); }

}  // namespace ref
