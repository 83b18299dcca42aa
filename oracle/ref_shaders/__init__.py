"""The reference's own shader arithmetic, compiled for the CPU - TEST INFRASTRUCTURE ONLY.

build() translates the reference checkout's sampler-free GLSL include files (translate.py), and compiles them with
glsl_compat.h and ref_entry.cpp into oracle/_ref/libref_shaders.so. oracle/_ref/ is ignored by git: the translated text
and the library are made from the reference and are never committed. Where the checkout is absent build() does nothing;
the tests then read the recorded results in tests/golden/ref_shader_kat.npz, which make_ref_shader_kat.py records from
this library.

The functions below call the library on whole arrays (float32 / uint32 / int32, one row per vector)."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import translate as _translate

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(_HERE, "..", "_ref")
CPP_PATH = os.path.join(OUT_DIR, "ref_shaders.cpp")
LIB_PATH = os.path.join(OUT_DIR, "libref_shaders.so")
CHECKOUT_ENV = "UTOPIAN_REFERENCE_DIR"
DEFAULT_CHECKOUT = "/root/reference"
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unused-but-set-variable"]
RESERVOIR_DTYPE = np.dtype([("Y", np.int32), ("W_sum", np.float32), ("W_X", np.float32), ("M", np.int32)])
LIGHT_FLOATS = 24  # color 4, pos 3, range, dir 3, spot, att 3, type, intensity 3, id, pad 4


def include_dir():
    """the reference checkout's shaders/include, or None where there is no checkout"""
    d = os.path.join(os.environ.get(CHECKOUT_ENV, DEFAULT_CHECKOUT), "utopian", "shaders", "include")
    return d if all(os.path.isfile(os.path.join(d, f)) for f in _translate.FILES) else None


def build(force=False):
    """-> LIB_PATH, or None where there is neither a checkout nor an earlier build"""
    inc = include_dir()
    if inc is None:
        return LIB_PATH if os.path.exists(LIB_PATH) else None
    sources = [os.path.join(inc, f) for f in _translate.FILES] + [os.path.join(_HERE, f) for f in ("glsl_compat.h", "ref_entry.cpp", "translate.py", "__init__.py")]
    if not force and os.path.exists(LIB_PATH) and os.path.exists(CPP_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in sources):
        return LIB_PATH
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(CPP_PATH, "w") as f:
        f.write(_translate.translate(inc))
    tmp = LIB_PATH + ".tmp%d" % os.getpid()
    subprocess.run([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-I", _HERE, "-I", OUT_DIR, "-shared", "-o", tmp, os.path.join(_HERE, "ref_entry.cpp")], check=True)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


_lib = None


def available():
    return os.path.exists(LIB_PATH) or include_dir() is not None


def lib():
    global _lib
    if _lib is None:
        path = build()
        if path is None:
            raise FileNotFoundError("no libref_shaders.so and no reference checkout (set %s)" % CHECKOUT_ENV)
        _lib = C.CDLL(path)
    return _lib


def _f(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def _u(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _call(name, n, *arrays):
    fn = getattr(lib(), name)
    fn.restype = None
    fn(C.c_int(n), *[C.c_void_p(a.ctypes.data) for a in arrays])


class Lights:
    """binds a lights buffer and view.num_lights / view.max_num_lights_used for the RIS functions. `lights` is (slots, 24)
    float32 and must hold every slot an index can reach: num_lights + 1 where a draw of exactly 1.0 occurs."""

    def __init__(self, lights, num_lights, max_num_lights_used):
        self.lights = _f(lights, LIGHT_FLOATS)
        self.num_lights, self.max_used = int(num_lights), int(max_num_lights_used)
        assert len(self.lights) > min(self.num_lights, self.max_used)

    def bind(self):
        fn = lib().ref_set_lights
        fn.restype = None
        fn(C.c_void_p(self.lights.ctypes.data), C.c_uint32(self.num_lights), C.c_uint32(self.max_used))


# ---- random.glsl -----------------------------------------------------------------------------------
def jenkins_hash(x):
    x = _u(x)
    out = np.empty_like(x)
    _call("ref_jenkins_hash", len(x), x, out)
    return out


def init_rng(px, py, resx, resy, frame):
    a = _u(np.stack(np.broadcast_arrays(_u(px), _u(py), _u(resx), _u(resy), _u(frame)), axis=-1), 5)
    out = np.empty(len(a), np.uint32)
    _call("ref_init_rng", len(a), a, out)
    return out


def random_float(state):
    """-> (values, states after)"""
    s = _u(state).copy()
    out = np.empty(len(s), np.float32)
    _call("ref_random_float", len(s), s, out)
    return out, s


def random_point_in_unit_sphere(state):
    s = _u(state).copy()
    out = np.empty((len(s), 3), np.float32)
    _call("ref_random_point_in_unit_sphere", len(s), s, out)
    return out, s


def random_point_in_unit_disk(state):
    s = _u(state).copy()
    out = np.empty((len(s), 2), np.float32)
    _call("ref_random_point_in_unit_disk", len(s), s, out)
    return out, s


# ---- restir_sampling.glsl --------------------------------------------------------------------------
def target_function(lights, light_index, hit_position):
    lights.bind()
    idx, p = _i(light_index), _f(hit_position, 3)
    out = np.empty(len(idx), np.float32)
    _call("ref_target_function", len(idx), idx, p, out)
    return out


def sample_light_uniform(lights, state):
    """-> (index, weight, states after)"""
    lights.bind()
    s = _u(state).copy()
    idx, w = np.empty(len(s), np.int32), np.empty(len(s), np.float32)
    _call("ref_sample_light_uniform", len(s), s, idx, w)
    return idx, w, s


def update_reservoir(state, reservoir, Xi, w_i, M):
    """-> (reservoirs after, states after)"""
    s = _u(state).copy()
    r = np.ascontiguousarray(reservoir, dtype=RESERVOIR_DTYPE).copy()
    _call("ref_update_reservoir", len(s), s, r, _i(Xi), _f(w_i), _i(M))
    return r, s


def finalize_resampling(reservoir, p_hat):
    r = np.ascontiguousarray(reservoir, dtype=RESERVOIR_DTYPE).copy()
    _call("ref_finalize_resampling", len(r), r, _f(p_hat))
    return r


def resample(lights, state, hit_position):
    """-> (reservoirs, states after)"""
    lights.bind()
    s, p = _u(state).copy(), _f(hit_position, 3)
    r = np.zeros(len(s), RESERVOIR_DTYPE)
    _call("ref_resample", len(s), s, p, r)
    return r, s


# ---- brdf.glsl, pbr_lighting.glsl ------------------------------------------------------------------
def distribution_ggx(N, H, roughness):
    N = _f(N, 3)
    out = np.empty(len(N), np.float32)
    _call("ref_distribution_ggx", len(N), N, _f(H, 3), _f(roughness), out)
    return out


def geometry_schlick_ggx(NdotV, roughness):
    x = _f(NdotV)
    out = np.empty(len(x), np.float32)
    _call("ref_geometry_schlick_ggx", len(x), x, _f(roughness), out)
    return out


def geometry_smith(N, V, L, roughness):
    N = _f(N, 3)
    out = np.empty(len(N), np.float32)
    _call("ref_geometry_smith", len(N), N, _f(V, 3), _f(L, 3), _f(roughness), out)
    return out


def fresnel_schlick(cos_theta, F0):
    c = _f(cos_theta)
    out = np.empty((len(c), 3), np.float32)
    _call("ref_fresnel_schlick", len(c), c, _f(F0, 3), out)
    return out


def fresnel_schlick_roughness(cos_theta, F0, roughness):
    c = _f(cos_theta)
    out = np.empty((len(c), 3), np.float32)
    _call("ref_fresnel_schlick_roughness", len(c), c, _f(F0, 3), _f(roughness), out)
    return out


def random(co):
    co = _f(co, 2)
    out = np.empty(len(co), np.float32)
    _call("ref_random", len(co), co, out)
    return out


def hammersley2d(i, N):
    a = _u(np.stack(np.broadcast_arrays(_u(i), _u(N)), axis=-1), 2)
    out = np.empty((len(a), 2), np.float32)
    _call("ref_hammersley2d", len(a), a, out)
    return out


def importance_sample_ggx(Xi, roughness, normal):
    Xi = _f(Xi, 2)
    out = np.empty((len(Xi), 3), np.float32)
    _call("ref_importance_sample_ggx", len(Xi), Xi, _f(roughness), _f(normal, 3), out)
    return out


def surface_shading(pixel, light, eye_pos, light_color_factor):
    """pixel (n, 11): position 3, baseColor 3, normal 3, metallic, roughness; light (n, 24); eye_pos (n, 3); factor (n,)"""
    pixel = _f(pixel, 11)
    out = np.empty((len(pixel), 3), np.float32)
    _call("ref_surface_shading", len(pixel), pixel, _f(light, LIGHT_FLOATS), _f(eye_pos, 3), _f(light_color_factor), out)
    return out


# ---- atmosphere.glsl -------------------------------------------------------------------------------
def sphere_intersection(ray_start, ray_dir, center, radius):
    s = _f(ray_start, 3)
    out = np.empty((len(s), 2), np.float32)
    _call("ref_sphere_intersection", len(s), s, _f(ray_dir, 3), _f(center, 3), _f(radius), out)
    return out


def phase_mie(costh, g):
    c = _f(costh)
    out = np.empty(len(c), np.float32)
    _call("ref_phase_mie", len(c), c, _f(g), out)
    return out


def integrate_optical_depth(ray_start, ray_dir):
    s = _f(ray_start, 3)
    out = np.empty((len(s), 3), np.float32)
    _call("ref_integrate_optical_depth", len(s), s, _f(ray_dir, 3), out)
    return out


def integrate_scattering(ray_start, ray_dir, ray_length, light_dir, light_color):
    """-> (color, transmittance)"""
    s = _f(ray_start, 3)
    color, tr = np.empty((len(s), 3), np.float32), np.empty((len(s), 3), np.float32)
    _call("ref_integrate_scattering", len(s), s, _f(ray_dir, 3), _f(ray_length), _f(light_dir, 3), _f(light_color, 3), color, tr)
    return color, tr
