"""Timing of uh_pose_mesh on one MI355X: a tube of about a million vertices (1,000 x 1,000 quads) with a skin of 64 joints and six morph
targets, four of them active, over a ground plane, device_build = 1. What it costs to show the next pose of the clip:

  route A  what a caller did before the verb: the pose computed on the host (tests/pose_reference.py, numpy float32), then
           uh_update_mesh_vertices(UH_VERTICES_HOST) + uh_refit_acceleration.
  route B  uh_update_mesh_vertices(UH_VERTICES_DEVICE) of vertices that are ready in a device buffer + the refit: the floor the library
           had - a check pass and a copy -, for a caller who has written a skinning kernel of their own.
  route C  uh_pose_mesh + the refit.

Host clock around each route, ending in uh_synchronize; an untimed pass of each first, then the routes alternate over the same
--phases, --rounds times over: medians and spreads. Beside them, from UhPoseStats::pose_ms (hipEvent around k_pose alone) on contexts
that hold the tube and no tree: the bytes the kernel must move (80 + 8 + 16 read and 80 written per vertex, 24 per vertex and active
target - normals are on) over its time, as a fraction of 8 TB/s, at 64 and at 1,024 joints; the host clock around the verb; and a
device-to-device copy of the vertex buffer, which is what copying the posed buffer over the mesh's own would add to exchanging them.
(profiles/pose_timing.json also holds the two variants that were measured with this tool and then deleted from the library: the copy,
and the joint matrices staged in LDS.) One JSON document, printed and written to --out.

  python tools/pose_timing.py [--grid 1000 --phases 5 --rounds 3 --out profiles/pose_timing.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pose_reference  # noqa: E402
import rust_renderer_amd as rr  # noqa: E402
from rust_renderer_amd.scenes import cylinder, quad  # noqa: E402

HBM_PEAK = 8.0e12
TARGETS, ACTIVE = 6, 4


def rig(grid, joints_n, seed=3):
    """the tube, its skin over joints_n joints along the axis (four nearest, smooth weights) and its targets"""
    v, idx = cylinder((0.0, 0.0, 0.0), 2.0, 40.0, grid, grid)
    rng = np.random.default_rng(seed)
    y = v["pos"][:, 1].astype(np.float64) / 40.0 * (joints_n - 1)
    first = np.clip(np.floor(y).astype(np.int64) - 1, 0, max(joints_n - 4, 0))
    joints = np.minimum(first[:, None] + np.arange(4)[None, :], joints_n - 1)
    w = np.exp(-((y[:, None] - joints) ** 2))
    weights = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    dp = (rng.uniform(-0.05, 0.05, (TARGETS, len(v), 3))).astype(np.float32)
    dn = (rng.uniform(-0.05, 0.05, (TARGETS, len(v), 3))).astype(np.float32)
    return v, idx, joints.astype(np.uint16), weights, dp, dn


def pose_inputs(joints_n, phase):
    """joint matrices that bend the tube as a travelling wave, and morph weights with TARGETS - ACTIVE exact zeros"""
    mats = np.zeros((joints_n, 3, 4))
    for j in range(joints_n):
        a = 0.05 * np.sin(0.3 * j + 0.7 * phase)
        c, s = np.cos(a), np.sin(a)
        mats[j, :, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        mats[j, :, 3] = [0.5 * np.sin(0.2 * j + phase), 0.0, 0.5 * np.cos(0.25 * j + phase)]
    mw = np.zeros(TARGETS, dtype=np.float32)
    mw[:ACTIVE] = 0.3 + 0.1 * np.cos(phase + np.arange(ACTIVE))
    return mats.astype(np.float32).reshape(joints_n, 12), mw


def clock(r, fn):
    r.synchronize()
    t0 = time.perf_counter()
    fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(samples):
    return dict(median=statistics.median(samples), min=min(samples), max=max(samples), spread=max(samples) - min(samples), samples=samples)


def kernel_bytes(n, skinned, active, normals=True):
    return n * (80 + 80 + (24 if skinned else 0) + active * (24 if normals else 12))


def lone_mesh(tube, joints_n, poses, repeats):
    """a context with the tube alone and no tree: (hipEvent ms of k_pose, host ms of the verb) over the poses, `repeats` times over"""
    v, idx, joints, weights, dp, dn = tube
    r = rr.Renderer(64, 64)
    mesh = r.add_mesh(v, idx, rr.make_material(diffuse_map=r.default_diffuse_map()))
    r.set_mesh_skin(mesh, joints, weights, joints_n)
    r.set_mesh_morph_targets(mesh, dp, dn)
    for jm, mw in poses[:2]:
        r.pose_mesh(mesh, jm, mw)  # warm-up: the code object, both vertex buffers
    kernel, verb = [], []
    for _ in range(repeats):
        for jm, mw in poses:
            verb.append(clock(r, lambda: r.pose_mesh(mesh, jm, mw)))
            kernel.append(r.pose_stats().pose_ms)
    s = r.pose_stats()
    out = dict(joints=joints_n, pose_ms=summary(kernel), verb_ms=summary(verb), staged_joint_limit=s.staged_joint_limit, device_bytes=s.device_bytes)
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--phases", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    J = 64
    tube = rig(a.grid, J)
    v, idx, joints, weights, dp, dn = tube
    n = len(v)
    poses = [pose_inputs(J, k + 1) for k in range(a.phases)]
    doc = dict(metric="pose", vertices=n, triangles=len(idx) // 3, joints=J, targets=TARGETS, active_targets=ACTIVE, device_build=1, phases=a.phases,
               rounds=a.rounds, library=rr.load_library().uh_version().decode())
    # ---- the three routes on a living context with a tree
    live = rr.Renderer(256, 256)
    live.set_option("device_build", 1)
    mat = rr.make_material(diffuse_map=live.default_diffuse_map())
    live.add_mesh(*quad((-60, -0.01, -60), (0, 0, 120), (120, 0, 0), 8, 8), mat)
    mesh = live.add_mesh(v, idx, mat)
    live.build_acceleration()
    live.set_mesh_skin(mesh, joints, weights, J)
    live.set_mesh_morph_targets(mesh, dp, dn)
    ready = [pose_reference.pose(v, joints, weights, jm, dp, dn, mw) for jm, mw in poses]
    hip = C.CDLL("libamdhip64.so.7")  # the runtime the library bound
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    buffers = []
    for p in ready:
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), p.nbytes) == 0 and hip.hipMemcpy(d, p.ctypes.data, p.nbytes, 1) == 0
        buffers.append(d.value)
    assert hip.hipDeviceSynchronize() == 0

    def route_a(k):
        def work():
            live.update_mesh_vertices(mesh, pose_reference.pose(v, joints, weights, poses[k][0], dp, dn, poses[k][1]))
            live.rebuild_tlas()
        return clock(live, work)

    def route_b(k):
        def work():
            live.update_mesh_vertices(mesh, device_ptr=buffers[k], count=n)
            live.rebuild_tlas()
        return clock(live, work)

    def route_c(k):
        def work():
            live.pose_mesh(mesh, *poses[k])
            live.rebuild_tlas()
        return clock(live, work)

    route_a(0), route_b(0), route_c(0)  # warm-up
    live.pose_mesh(mesh, *poses[-1])
    assert live.read_mesh(mesh)[0].tobytes() == ready[-1].tobytes(), "k_pose and the host reference differ at the size that is timed"
    live.rebuild_tlas()
    sa, sb, sc, kernel, gather, refit = [], [], [], [], [], []
    for _ in range(a.rounds):
        for k in range(a.phases):
            sa.append(route_a(k))
            sb.append(route_b(k))
            sc.append(route_c(k))
            kernel.append(live.pose_stats().pose_ms)
            u = live.mesh_update_stats()
            gather.append(u.gather_ms), refit.append(u.refit_ms)
    need = kernel_bytes(n, True, ACTIVE)
    doc.update(route_a_ms=summary(sa), route_b_ms=summary(sb), route_c_ms=summary(sc), pose_ms=summary(kernel), gather_ms=summary(gather),
               refit_ms=summary(refit), kernel_bytes=need, kernel_bytes_per_second=need / (statistics.median(kernel) * 1e-3),
               kernel_fraction_of_hbm_peak=need / (statistics.median(kernel) * 1e-3) / HBM_PEAK,
               route_b_copy_bytes=2 * 80 * n + 12 * n, c_over_b=statistics.median(sc) / statistics.median(sb), a_over_c=statistics.median(sa) / statistics.median(sc),
               host_geometry_bytes=live.mesh_update_stats().host_geometry_bytes)
    live.close()
    # what copying the posed buffer over the mesh's own would add to a pose that exchanges them: 80 bytes per vertex, device to device
    hip.hipDeviceSynchronize()
    copies = []
    for k in range(4 * a.rounds):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(buffers[0], buffers[1], ready[0].nbytes, 3) == 0 and hip.hipDeviceSynchronize() == 0
        copies.append((time.perf_counter() - t0) * 1e3)
    doc["vertex_buffer_copy_ms"] = summary(copies[a.rounds:])
    for d in buffers:
        hip.hipFree(d)
    # ---- the kernel's variants, on contexts without a tree
    repeats = 2 * a.rounds
    doc["joints_64"] = lone_mesh(tube, J, poses, repeats)
    wide = rig(a.grid, 1024)
    doc["joints_1024"] = lone_mesh(wide, 1024, [pose_inputs(1024, k + 1) for k in range(a.phases)], repeats)
    line = json.dumps(doc)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
