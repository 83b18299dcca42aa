"""glTF 2.0 ingestion on the caller side of the boundary: turns a
.gltf file into the `scenes.Model` that `Renderer.add_model` uploads, with the semantics of the
reference's loader (utopian/src/gltf_loader.rs:47-218):

* nodes are walked depth first, children BEFORE the node's own mesh (gltf_loader.rs:57-63), the
  node transform is parent * local, one Mesh + one transform per primitive;
* Vertex{pos.w = 0, normal.w = 0, uv (0,0) if absent, color (1,1,1,1) if absent, tangent 0 if absent};
* material: base colour factor / metallic / roughness; diffuse_map = the glTF *texture* index used to
  index the model's *image* list (the reference's own quirk, gltf_loader.rs:103-107 vs :183-207);
  material_type Lambertian, property 0 (callers override, e.g. scenes.rs:116-121);
* images become RGBA8 (RGB8 is expanded, anything else is the reference's "Unsupported image format!",
  gltf_loader.rs:179-198); PNG is decoded in-repo (image_decode.py), JPEG needs Pillow (optional).
Buffers may be base64 data URIs or files next to the .gltf.
Beyond the reference's loader (which draws every asset in its bind pose): skins, morph targets and animation clips. A primitive with
JOINTS_0 / WEIGHTS_0 or `targets` carries them in the Mesh's optional fields, the Model carries `skins`, `animations` and `nodes`;
everything the loader returned before is unchanged, a skinned primitive's `transform` included. `Animator` samples a clip with the
semantics of the glTF 2.0 specification and poses the meshes through Renderer.pose_mesh (include/utopian_hip.h "posed meshes").
`instance_transform_3x4` applies the scale-rotation-translation round trip of
Raytracing::fill_instance_array (raytracing.rs:229-248), which drops shear.
"""
import base64
import json
import os
from dataclasses import dataclass, field

import numpy as np

from .image_decode import load_image_rgba8
from .scenes import Mesh, Model
from .types import LAMBERTIAN, VERTEX_DTYPE

f32 = np.float32
_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_NUM = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


@dataclass
class Node:
    """a glTF node: its static local transform as TRS (or `matrix`, 4x4 row-major float64, when the file gives one) and its links"""
    name: str = ""
    parent: int = None
    children: list = field(default_factory=list)
    translation: np.ndarray = None  # (3,) float64
    rotation: np.ndarray = None     # (4,) float64, xyzw
    scale: np.ndarray = None        # (3,) float64
    matrix: np.ndarray = None
    mesh: int = None
    skin: int = None
    weights: np.ndarray = None      # (T,) float64: the node's own morph weights, None when absent


@dataclass
class Skin:
    joints: list                    # node indices
    inverse_bind: np.ndarray        # (J, 4, 4) float64, row-major; identities when the file has no inverseBindMatrices
    skeleton: int = None
    name: str = ""


@dataclass
class AnimationSampler:
    times: np.ndarray               # (K,) float64, ascending
    values: np.ndarray              # (K, C) float64; CUBICSPLINE: (K, 3, C) - in-tangent, value, out-tangent
    interpolation: str = "LINEAR"


@dataclass
class AnimationChannel:
    node: int
    path: str                       # translation | rotation | scale | weights
    sampler: int


@dataclass
class Animation:
    name: str = ""
    samplers: list = field(default_factory=list)
    channels: list = field(default_factory=list)


def _load_uri(uri, base_dir):
    if uri.startswith("data:"):
        return base64.b64decode(uri.split(",", 1)[1])
    with open(os.path.join(base_dir, uri), "rb") as f:
        return f.read()


def _accessor(gltf, buffers, index, as_float=False):
    acc = gltf["accessors"][index]
    if "sparse" in acc:
        raise NotImplementedError("sparse accessors")
    dt, n, count = np.dtype(_COMPONENT[acc["componentType"]]), _NUM[acc["type"]], acc["count"]
    if "bufferView" not in acc:
        out = np.zeros((count, n), dtype=dt)
    else:
        bv = gltf["bufferViews"][acc["bufferView"]]
        raw = buffers[bv["buffer"]]
        start = bv.get("byteOffset", 0) + acc.get("byteOffset", 0)
        stride = bv.get("byteStride", 0) or dt.itemsize * n
        out = np.ndarray((count, n), dtype=dt, buffer=raw, offset=start, strides=(stride, dt.itemsize)).copy()
    if as_float and dt != np.float32:
        scale = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0, np.dtype(np.int8): 127.0, np.dtype(np.int16): 32767.0}.get(dt)
        out = out.astype(f32) / f32(scale) if acc.get("normalized") and scale else out.astype(f32)
    return out


def _quat_to_mat3(q):
    x, y, z, w = (f32(v) for v in q)
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz, wx, wy, wz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2, w * x2, w * y2, w * z2
    return np.array([[1 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1 - (xx + yy)]], dtype=f32)


def _node_matrix(node):
    if "matrix" in node:
        return np.array(node["matrix"], dtype=f32).reshape(4, 4).T  # glTF stores column-major
    m = np.eye(4, dtype=f32)
    r = _quat_to_mat3(node.get("rotation", [0, 0, 0, 1]))
    s = np.array(node.get("scale", [1, 1, 1]), dtype=f32)
    m[:3, :3] = r * s[None, :]
    m[:3, 3] = np.array(node.get("translation", [0, 0, 0]), dtype=f32)
    return m


def load_gltf(path):
    """utopian::gltf_loader::load_gltf -> Model (textures as (H, W, 4) uint8 arrays)."""
    base_dir = os.path.dirname(os.path.abspath(path))
    with open(path) as f:
        gltf = json.load(f)
    buffers = [_load_uri(b["uri"], base_dir) for b in gltf.get("buffers", [])]
    model = Model([], [])
    for image in gltf.get("images", []):
        data = _load_uri(image["uri"], base_dir) if "uri" in image else bytes(
            buffers[gltf["bufferViews"][image["bufferView"]]["buffer"]][
                gltf["bufferViews"][image["bufferView"]].get("byteOffset", 0):][: gltf["bufferViews"][image["bufferView"]]["byteLength"]]
        )
        model.textures.append(load_image_rgba8(bytes(data)))

    def load_node(index, parent):
        node = gltf["nodes"][index]
        transform = (parent @ _node_matrix(node)).astype(f32)
        for child in node.get("children", []):
            load_node(child, transform)
        if "mesh" not in node:
            return
        for prim in gltf["meshes"][node["mesh"]]["primitives"]:
            attrs = prim["attributes"]
            pos = _accessor(gltf, buffers, attrs["POSITION"], True)
            nrm = _accessor(gltf, buffers, attrs["NORMAL"], True)
            idx = _accessor(gltf, buffers, prim["indices"]).astype(np.uint32).reshape(-1)
            v = np.zeros(len(pos), dtype=VERTEX_DTYPE)
            v["pos"][:, :3] = pos
            v["normal"][:, :3] = nrm
            if "TEXCOORD_0" in attrs:
                v["uv"] = _accessor(gltf, buffers, attrs["TEXCOORD_0"], True)
            if "TANGENT" in attrs:
                v["tangent"] = _accessor(gltf, buffers, attrs["TANGENT"], True)
            v["color"] = 1.0
            if "COLOR_0" in attrs:
                c = _accessor(gltf, buffers, attrs["COLOR_0"], True)
                v["color"][:, : c.shape[1]] = c
            rig = _primitive_rig(gltf, buffers, node, prim, len(pos))
            mat = gltf["materials"][prim["material"]] if "material" in prim else {}
            pbr = mat.get("pbrMetallicRoughness", {})
            tex = pbr.get("baseColorTexture", {}).get("index")
            mesh = Mesh(v, idx, LAMBERTIAN, 0.0, tuple(float(x) for x in pbr.get("baseColorFactor", [1, 1, 1, 1])), tex, transform[:3, :].reshape(12).copy(),
                        name=mat.get("name", node.get("name", "")), metallic=float(pbr.get("metallicFactor", 1.0)), roughness=float(pbr.get("roughnessFactor", 1.0)), node=index, **rig)
            model.meshes.append(mesh)

    scenes = gltf.get("scenes", [])
    for scene in scenes:
        for n in scene.get("nodes", []):
            load_node(n, np.eye(4, dtype=f32))
    _load_rig(gltf, buffers, model)
    return model


def _primitive_rig(gltf, buffers, node, prim, n):
    """the optional Mesh fields of a primitive: JOINTS_0 / WEIGHTS_0 (with the node's skin) and the morph targets"""
    attrs, rig = prim["attributes"], {}
    if "JOINTS_1" in attrs or "WEIGHTS_1" in attrs:
        raise NotImplementedError("JOINTS_1 / WEIGHTS_1: more than four influences per vertex")
    if "JOINTS_0" in attrs and "WEIGHTS_0" in attrs and "skin" in node:
        rig.update(joints=_accessor(gltf, buffers, attrs["JOINTS_0"]).astype(np.uint16), weights=_accessor(gltf, buffers, attrs["WEIGHTS_0"], True).astype(f32),
                   skin=int(node["skin"]))
    targets = prim.get("targets", [])
    if targets and all("POSITION" in t for t in targets):
        rig["morph_positions"] = np.stack([_accessor(gltf, buffers, t["POSITION"], True) for t in targets]).astype(f32)
        if all("NORMAL" in t for t in targets):
            rig["morph_normals"] = np.stack([_accessor(gltf, buffers, t["NORMAL"], True) for t in targets]).astype(f32)
        w = gltf["meshes"][node["mesh"]].get("weights")
        rig["morph_default_weights"] = np.zeros(len(targets), dtype=f32) if w is None else np.array(w, dtype=f32)
        assert rig["morph_positions"].shape == (len(targets), n, 3)
    return rig


def _load_rig(gltf, buffers, model):
    """Model.nodes / skins / animations"""
    for n in gltf.get("nodes", []):
        node = Node(name=n.get("name", ""), children=list(n.get("children", [])), mesh=n.get("mesh"), skin=n.get("skin"),
                    translation=np.array(n.get("translation", [0, 0, 0]), dtype=np.float64), rotation=np.array(n.get("rotation", [0, 0, 0, 1]), dtype=np.float64),
                    scale=np.array(n.get("scale", [1, 1, 1]), dtype=np.float64), weights=None if "weights" not in n else np.array(n["weights"], dtype=np.float64))
        if "matrix" in n:
            node.matrix = np.array(n["matrix"], dtype=np.float64).reshape(4, 4).T
        model.nodes.append(node)
    for i, node in enumerate(model.nodes):
        for c in node.children:
            model.nodes[c].parent = i
    for s in gltf.get("skins", []):
        joints = [int(j) for j in s["joints"]]
        if "inverseBindMatrices" in s:
            ibm = _accessor(gltf, buffers, s["inverseBindMatrices"], True).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)  # column-major in the file
        else:
            ibm = np.tile(np.eye(4), (len(joints), 1, 1))
        assert len(ibm) == len(joints)
        model.skins.append(Skin(joints, np.ascontiguousarray(ibm), s.get("skeleton"), s.get("name", "")))
    for a in gltf.get("animations", []):
        anim = Animation(a.get("name", ""))
        for smp in a.get("samplers", []):
            times = _accessor(gltf, buffers, smp["input"], True).astype(np.float64).reshape(-1)
            values = _accessor(gltf, buffers, smp["output"], True).astype(np.float64)
            anim.samplers.append(AnimationSampler(times, values, smp.get("interpolation", "LINEAR")))
        for ch in a.get("channels", []):
            if "node" not in ch["target"]:
                continue  # (the specification: a channel without a target node is ignored)
            anim.channels.append(AnimationChannel(int(ch["target"]["node"]), ch["target"]["path"], int(ch["sampler"])))
        for ch in anim.channels:  # a sampler's output is (keys, components of its channel's path), three per key for CUBICSPLINE
            smp = anim.samplers[ch.sampler]
            if smp.values.ndim == 2:
                k = len(smp.times)
                smp.values = smp.values.reshape((k, 3, -1) if smp.interpolation == "CUBICSPLINE" else (k, -1))
        model.animations.append(anim)


def _trs(translation, rotation, scale):
    """T * R * S as a 4x4, float64"""
    x, y, z, w = rotation
    m = np.eye(4)
    m[:3, :3] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]) * np.asarray(scale)[None, :]
    m[:3, 3] = translation
    return m


def _slerp(a, b, u):
    """between unit quaternions on the shortest arc, renormalised"""
    d = float(np.dot(a, b))
    if d < 0.0:
        b, d = -b, -d
    if d > 0.9995:  # nearly parallel: the sine form loses its digits, the chord is the arc
        q = a + u * (b - a)
    else:
        th = np.arccos(d)
        q = (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)
    return q / np.linalg.norm(q)


def sample(sampler, t, rotation=False):
    """the sampler's value at time t (clamped to its first and last key), float64: LINEAR (slerp for rotations), STEP or CUBICSPLINE.
    A rotation is a unit quaternion whatever the file's float32 keys add up to: keys are normalised before they are used or blended on the
    sphere, a spline's result after it is formed (the specification's rule)"""
    times, values = sampler.times, sampler.values
    cubic = sampler.interpolation == "CUBICSPLINE"
    unit = (lambda q: q / np.linalg.norm(q)) if rotation else (lambda v: v.copy())
    key = (lambda k: unit(values[k, 1])) if cubic else (lambda k: unit(values[k]))
    t = min(max(float(t), times[0]), times[-1])
    if len(times) == 1 or t >= times[-1]:
        return key(len(times) - 1)
    i = int(np.searchsorted(times, t, side="right")) - 1
    dt = times[i + 1] - times[i]
    u = (t - times[i]) / dt
    if sampler.interpolation == "STEP":
        return key(i)
    if cubic:
        u2, u3 = u * u, u * u * u
        return unit((2 * u3 - 3 * u2 + 1) * values[i, 1] + dt * (u3 - 2 * u2 + u) * values[i, 2] + (-2 * u3 + 3 * u2) * values[i + 1, 1] + dt * (u3 - u2) * values[i + 1, 0])
    if rotation:
        return _slerp(key(i), key(i + 1), u)
    return values[i] + u * (values[i + 1] - values[i])


class Animator:
    """Poses the rigged meshes of a Model of load_gltf at a time of one of its animation clips, with the semantics of the glTF 2.0
    specification: channels target a node's translation, rotation, scale or morph weights; a property no channel targets keeps the
    node's static value; global transforms are parent * local over the whole hierarchy; a skinned mesh's joint matrix k is
    inverse(G_meshnode) @ G_joint(k) @ inverseBind(k), G_meshnode the rest-pose global transform of the node that carries the mesh -
    the instance transform the mesh was added with -, so that the renderer's transform times the joint matrix places a vertex where
    the specification does: at G_joint @ inverseBind @ v, whatever the mesh's node does. Computed in float64, rounded once."""

    def __init__(self, model):
        self.model = model
        self.posable = [i for i, m in enumerate(model.meshes) if m.skin is not None or m.morph_positions is not None]
        self._rest = self.globals(None, 0.0)[0]

    def locals_at(self, animation, t):
        """([4x4 local transform of every node], {node: morph weights}) at time t of clip `animation` (index, or None: the static scene)"""
        nodes = self.model.nodes
        trs = [dict(translation=n.translation, rotation=n.rotation, scale=n.scale) for n in nodes]
        animated, weights = set(), {}
        if animation is not None:
            clip = self.model.animations[animation]
            for ch in clip.channels:
                value = sample(clip.samplers[ch.sampler], t, rotation=ch.path == "rotation")
                if ch.path == "weights":
                    weights[ch.node] = value
                else:
                    trs[ch.node][ch.path] = value
                    animated.add(ch.node)
        return [n.matrix if n.matrix is not None and i not in animated else _trs(**trs[i]) for i, n in enumerate(nodes)], weights

    def globals(self, animation, t):
        local, weights = self.locals_at(animation, t)
        out = [None] * len(local)

        def visit(i, parent):
            out[i] = parent @ local[i]
            for c in self.model.nodes[i].children:
                visit(c, out[i])

        for i, n in enumerate(self.model.nodes):
            if n.parent is None:
                visit(i, np.eye(4))
        return out, weights

    def pose(self, animation, t):
        """{index into model.meshes: (joint_matrices (J, 12) float32 | None, morph_weights (T,) float32 | None)} for every skinned or
        morphed mesh, at time t of clip `animation`"""
        g, weights = self.globals(animation, t)
        out = {}
        for i in self.posable:
            m = self.model.meshes[i]
            jm = mw = None
            if m.skin is not None:
                skin = self.model.skins[m.skin]
                to_mesh = np.linalg.inv(self._rest[m.node])
                jm = np.stack([(to_mesh @ g[j] @ skin.inverse_bind[k])[:3, :].reshape(12) for k, j in enumerate(skin.joints)]).astype(f32)
            if m.morph_positions is not None:
                node = self.model.nodes[m.node]
                w = weights.get(m.node, node.weights if node.weights is not None else m.morph_default_weights)
                mw = np.asarray(w, dtype=np.float64).astype(f32)
            out[i] = (jm, mw)
        return out

    def apply(self, renderer, mesh_ids, animation, t):
        """poses the meshes `mesh_ids` (what renderer.add_model(model) returned) at time t; a refit or a build has to follow"""
        for i, (jm, mw) in self.pose(animation, t).items():
            renderer.pose_mesh(mesh_ids[i], jm, mw)


def load_cube():
    """ModelLoader::load_cube (utopian/src/model_loader.rs:65-156): unit cube, 24 vertices, the
    reference's own face / normal / uv assignment (its "Top" face carries the -y normal)."""
    faces = [  # (normal, four corners in the reference's vertex order), uv = (0,1) (1,1) (1,0) (0,0)
        ((0, 0, 1), [(-.5, -.5, .5), (.5, -.5, .5), (.5, .5, .5), (-.5, .5, .5)]),
        ((0, 0, -1), [(-.5, -.5, -.5), (.5, -.5, -.5), (.5, .5, -.5), (-.5, .5, -.5)]),
        ((0, -1, 0), [(-.5, -.5, -.5), (.5, -.5, -.5), (.5, -.5, .5), (-.5, -.5, .5)]),
        ((0, 1, 0), [(-.5, .5, -.5), (.5, .5, -.5), (.5, .5, .5), (-.5, .5, .5)]),
        ((-1, 0, 0), [(-.5, -.5, -.5), (-.5, .5, -.5), (-.5, .5, .5), (-.5, -.5, .5)]),
        ((1, 0, 0), [(.5, -.5, -.5), (.5, .5, -.5), (.5, .5, .5), (.5, -.5, .5)]),
    ]
    uvs = [(0, 1), (1, 1), (1, 0), (0, 0)]
    v = np.zeros(24, dtype=VERTEX_DTYPE)
    for fi, (n, corners) in enumerate(faces):
        for ci, p in enumerate(corners):
            k = fi * 4 + ci
            v["pos"][k, :3], v["normal"][k, :3], v["uv"][k], v["color"][k] = p, n, uvs[ci], 1.0
    winding = [(2, 0, 1, 0, 2, 3), (0, 2, 1, 2, 0, 3)]  # front/top/right vs back/bottom/left pattern of model_loader.rs:76-99
    idx = []
    for fi, pat in enumerate([0, 1, 0, 1, 1, 0]):
        idx += [fi * 4 + o for o in winding[pat]]
    return Model([Mesh(v, np.array(idx, dtype=np.uint32), LAMBERTIAN, 0.0, (1.0, 1.0, 1.0, 1.0), None, name="cube")], [])


def instance_transform_3x4(world4x4):
    """instance.transform * model.transforms[i] -> to_scale_rotation_translation -> recomposed 3x4
    (raytracing.rs:229-248): scale = column lengths (x negated for a negative determinant),
    rotation = normalised columns through a quaternion, shear is lost."""
    m = np.asarray(world4x4, dtype=f32).reshape(4, 4) if np.size(world4x4) == 16 else np.vstack([np.asarray(world4x4, dtype=f32).reshape(3, 4), [0, 0, 0, 1]]).astype(f32)
    a = m[:3, :3].astype(np.float64)
    det = np.linalg.det(a)
    s = np.linalg.norm(a, axis=0)
    if det < 0:
        s[0] = -s[0]
    r = a / np.where(s == 0, 1.0, s)[None, :]
    # Mat3 -> Quat -> Mat3 (orthonormalises what is left)
    t = np.trace(r)
    if t > 0:
        w = np.sqrt(1 + t) / 2
        q = np.array([(r[2, 1] - r[1, 2]) / (4 * w), (r[0, 2] - r[2, 0]) / (4 * w), (r[1, 0] - r[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(r)))
        j, k = (i + 1) % 3, (i + 2) % 3
        x = np.sqrt(max(1 + r[i, i] - r[j, j] - r[k, k], 0.0)) / 2
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = x, (r[j, i] + r[i, j]) / (4 * x), (r[k, i] + r[i, k]) / (4 * x), (r[k, j] - r[j, k]) / (4 * x)
    q /= np.linalg.norm(q)
    out = np.zeros((3, 4), dtype=f32)
    out[:, :3] = _quat_to_mat3(q) * s.astype(f32)[None, :]
    out[:, 3] = m[:3, 3]
    return out.reshape(12)
