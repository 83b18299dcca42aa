// pose.hip — posed meshes (utopian_hip.h "posed meshes"): uh_set_mesh_skin and uh_set_mesh_morph_targets keep a mesh's bind pose, its
// skin and its morph targets on the device; uh_pose_mesh writes the mesh's vertices from them with one kernel, k_pose, and hands the
// result to the path uh_update_mesh_vertices(UH_VERTICES_DEVICE) takes (scene_build.hip replace_mesh_vertices): the refit, the motion
// vectors and every graph follow from there. The arithmetic is DESIGN.md section 2 "Posed meshes"; tests/pose_reference.py restates it.
//
// k_pose is one thread per vertex and bandwidth bound: the bind record as five 16-byte loads, 8 bytes of joints and 16 of weights, 12
// (24 with normals) per ACTIVE target - the host passes only the targets whose weight is not zero, so the loop's trip count is the
// grid's -, the record out as five 16-byte stores. The deltas are target-major: a wave's 64 x 12 bytes of one target are contiguous.
// The call's joint matrices (48 bytes each) are read through L2 as they are: staging them in LDS per block measured the same at 64
// joints and a third slower at 1,024 (DESIGN.md section 4 "Posed meshes"), and swapping the second vertex buffer in beat copying it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context_state.h"
#include "device_types.h"
#include "utopian_hip.h"

using namespace uh;

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxJoints = 65536;       // joint indices are 16 bits
static_assert(sizeof(UhVertex) == 80, "five 16-byte quads: pos, normal, uv + pad, color, tangent");

struct PoseArgs {
   const float4* bind;     // 5 per vertex
   float4* out;            // 5 per vertex
   const uint2* joints;    // four 16-bit indices per vertex
   const float4* weights;  // one per vertex
   const float4* mats;     // 3 per joint: the rows of its 3x4
   const uint2* active;    // (target, bits of its weight) of the targets whose weight is not zero, ascending
   const float* dpos;      // 3 per target and vertex, target-major
   const float* dnrm;      // the same shape, or null
   uint32_t* flag;         // |= 1 when a posed position is not finite
   uint32_t num_vertices, num_joints, num_active;
};

// v unchanged if it is zero, else v * (1 / sqrt(dot(v, v))): normalize3 of device_math.h behind a zero test
__device__ __forceinline__ void normalize_or_keep(float& x, float& y, float& z) {
   const float d = (x * x + y * y) + z * z;
   if (d == 0.0f) return;
   const float inv = 1.0f / sqrtf(d);
   x = x * inv, y = y * inv, z = z * inv;
}

template <bool kSkin>
__global__ __launch_bounds__(kBlock) void k_pose(const PoseArgs a) {
   const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
   bool bad = false;
   if (i < a.num_vertices) {
      const float4* b = a.bind + 5 * (size_t)i;
      float4 pos = b[0], nrm = b[1], tan = b[4];
      const float4 uv = b[2], col = b[3];
      // morph: the active targets in ascending order, product then sum
      for (uint32_t k = 0; k < a.num_active; k++) {
         const uint2 t = a.active[k];
         const float w = __uint_as_float(t.y);
         const size_t at = 3 * ((size_t)t.x * a.num_vertices + i);
         const float* dp = a.dpos + at;
         pos.x = pos.x + w * dp[0], pos.y = pos.y + w * dp[1], pos.z = pos.z + w * dp[2];
         if (a.dnrm) {
            const float* dn = a.dnrm + at;
            nrm.x = nrm.x + w * dn[0], nrm.y = nrm.y + w * dn[1], nrm.z = nrm.z + w * dn[2];
         }
      }
      if (kSkin) {
         const uint2 jj = a.joints[i];
         const float4 w = a.weights[i];
         const uint32_t j0 = jj.x & 0xffffu, j1 = jj.x >> 16, j2 = jj.y & 0xffffu, j3 = jj.y >> 16;
         float4 m[3];
         for (int r = 0; r < 3; r++) {
            const float4 A0 = a.mats[3 * j0 + r];
            const float4 A1 = a.mats[3 * j1 + r];
            const float4 A2 = a.mats[3 * j2 + r];
            const float4 A3 = a.mats[3 * j3 + r];
            m[r].x = ((w.x * A0.x + w.y * A1.x) + w.z * A2.x) + w.w * A3.x;
            m[r].y = ((w.x * A0.y + w.y * A1.y) + w.z * A2.y) + w.w * A3.y;
            m[r].z = ((w.x * A0.z + w.y * A1.z) + w.z * A2.z) + w.w * A3.z;
            m[r].w = ((w.x * A0.w + w.y * A1.w) + w.z * A2.w) + w.w * A3.w;
         }
         const float px = pos.x, py = pos.y, pz = pos.z, nx = nrm.x, ny = nrm.y, nz = nrm.z, tx = tan.x, ty = tan.y, tz = tan.z;
         pos.x = ((m[0].x * px + m[0].y * py) + m[0].z * pz) + m[0].w;
         pos.y = ((m[1].x * px + m[1].y * py) + m[1].z * pz) + m[1].w;
         pos.z = ((m[2].x * px + m[2].y * py) + m[2].z * pz) + m[2].w;
         nrm.x = (m[0].x * nx + m[0].y * ny) + m[0].z * nz;
         nrm.y = (m[1].x * nx + m[1].y * ny) + m[1].z * nz;
         nrm.z = (m[2].x * nx + m[2].y * ny) + m[2].z * nz;
         tan.x = (m[0].x * tx + m[0].y * ty) + m[0].z * tz;
         tan.y = (m[1].x * tx + m[1].y * ty) + m[1].z * tz;
         tan.z = (m[2].x * tx + m[2].y * ty) + m[2].z * tz;
         normalize_or_keep(tan.x, tan.y, tan.z);
      }
      normalize_or_keep(nrm.x, nrm.y, nrm.z);
      bad = !isfinite(pos.x) || !isfinite(pos.y) || !isfinite(pos.z);
      float4* o = a.out + 5 * (size_t)i;
      o[0] = pos, o[1] = nrm, o[2] = uv, o[3] = col, o[4] = tan;
   }
   if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(a.flag, 1u);
}

void launch_pose(hipStream_t stream, const PoseArgs& a) {
   const uint32_t blocks = (a.num_vertices + kBlock - 1) / kBlock;
   if (a.num_joints)
      k_pose<true><<<blocks, kBlock, 0, stream>>>(a);
   else
      k_pose<false><<<blocks, kBlock, 0, stream>>>(a);
}

// a fresh device copy of `bytes` host bytes; null (and *e set) when it cannot be made
void* device_copy_of(const void* host, size_t bytes, hipError_t* e) {
   void* d = nullptr;
   if ((*e = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
   if ((*e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)) != hipSuccess) {
      (void)hipFree(d);
      return nullptr;
   }
   return d;
}

// the mesh's current vertices in a fresh device buffer: the bind pose of a set verb
UhVertex* take_bind_pose(uh_ctx* c, const HostMesh& m, hipError_t* e) {
   const size_t bytes = m.vertices.size() * sizeof(UhVertex);
   if (m.upd && !m.host_valid) {  // the host copy is stale: the mesh's own device buffer has them
      void* d = nullptr;
      if ((*e = hipMalloc(&d, bytes)) != hipSuccess) return nullptr;
      if ((*e = hipMemcpy(d, m.d_verts, bytes, hipMemcpyDeviceToDevice)) != hipSuccess || (*e = hipDeviceSynchronize()) != hipSuccess) {
         (void)hipFree(d);
         return nullptr;
      }
      return static_cast<UhVertex*>(d);
   }
   UhVertex* d = static_cast<UhVertex*>(device_copy_of(m.vertices.data(), bytes, e));
   if (d && m.upd) c->mupd.st.host_geometry_bytes += bytes;
   return d;
}

// what the three verbs refuse alike; the mesh otherwise
int posable_mesh(uh_ctx* c, uint32_t mesh_index, const std::string& verb, HostMesh** out) {
   if (mesh_index >= c->meshes.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": bad mesh index");
   HostMesh& m = c->meshes[mesh_index];
   if (m.iso) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": the mesh was created by uh_add_isosurface_mesh");
   if (m.vertices.empty()) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": the mesh has no vertices");
   *out = &m;
   return UH_OK;
}

int hip_refusal(uh_ctx* c, const std::string& verb, hipError_t e) {
   return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, verb + ": the mesh's device buffers: " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int uh_set_mesh_skin(uh_ctx* c, uint32_t mesh_index, const uint16_t* joints, const float* weights, uint32_t num_vertices, uint32_t num_joints) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const std::string verb = "uh_set_mesh_skin";
   HostMesh* mp = nullptr;
   if (int st = posable_mesh(c, mesh_index, verb, &mp)) return st;
   HostMesh& m = *mp;
   if (num_vertices != m.vertices.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": the vertex count differs from the mesh's");
   if (!num_joints || num_joints > kMaxJoints) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": num_joints must be 1..65536");
   if (!joints || !weights) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": null joints or weights");
   for (size_t i = 0; i < num_vertices; i++) {
      bool any = false;
      for (int k = 0; k < 4; k++) {
         const float w = weights[4 * i + k];
         if (joints[4 * i + k] >= num_joints) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": joint index out of range");
         if (!std::isfinite(w) || w < 0.0f) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": a weight is negative or not finite");
         any = any || w != 0.0f;
      }
      if (!any) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": a vertex has four zero weights");
   }
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   // the new buffers first: a refusal leaves the mesh as it was
   hipError_t e = hipSuccess;
   UhVertex* bind = take_bind_pose(c, m, &e);
   uint16_t* dj = bind ? static_cast<uint16_t*>(device_copy_of(joints, 4 * (size_t)num_vertices * sizeof(uint16_t), &e)) : nullptr;
   float* dw = dj ? static_cast<float*>(device_copy_of(weights, 4 * (size_t)num_vertices * sizeof(float), &e)) : nullptr;
   if (!dw) {
      for (void* p : {(void*)bind, (void*)dj})
         if (p) (void)hipFree(p);
      return hip_refusal(c, verb, e);
   }
   if (!m.pose) m.pose = new MeshPose;
   MeshPose& p = *m.pose;
   for (void* old : {(void*)p.bind, (void*)p.joints, (void*)p.weights})
      if (old) (void)hipFree(old);
   p.bind = bind, p.joints = dj, p.weights = dw, p.num_joints = num_joints;
   return UH_OK;
}

int uh_set_mesh_morph_targets(uh_ctx* c, uint32_t mesh_index, const float* position_deltas, const float* normal_deltas, uint32_t num_vertices,
                              uint32_t num_targets) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const std::string verb = "uh_set_mesh_morph_targets";
   HostMesh* mp = nullptr;
   if (int st = posable_mesh(c, mesh_index, verb, &mp)) return st;
   HostMesh& m = *mp;
   if (num_vertices != m.vertices.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": the vertex count differs from the mesh's");
   if (!num_targets) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": num_targets must not be 0");
   if (!position_deltas) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": null position deltas");
   const size_t count = 3 * (size_t)num_targets * num_vertices;
   for (const float* d : {position_deltas, normal_deltas})
      for (size_t i = 0; d && i < count; i++)
         if (!std::isfinite(d[i])) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": a delta is not finite");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   hipError_t e = hipSuccess;
   UhVertex* bind = take_bind_pose(c, m, &e);
   float* dp = bind ? static_cast<float*>(device_copy_of(position_deltas, count * sizeof(float), &e)) : nullptr;
   float* dn = dp && normal_deltas ? static_cast<float*>(device_copy_of(normal_deltas, count * sizeof(float), &e)) : nullptr;
   if (!dp || (normal_deltas && !dn)) {
      for (void* p : {(void*)bind, (void*)dp})
         if (p) (void)hipFree(p);
      return hip_refusal(c, verb, e);
   }
   if (!m.pose) m.pose = new MeshPose;
   MeshPose& p = *m.pose;
   for (void* old : {(void*)p.bind, (void*)p.dpos, (void*)p.dnrm})
      if (old) (void)hipFree(old);
   p.bind = bind, p.dpos = dp, p.dnrm = dn, p.num_targets = num_targets;
   return UH_OK;
}

int uh_pose_mesh(uh_ctx* c, uint32_t mesh_index, const float* joint_matrices3x4, uint32_t num_joints, const float* morph_weights, uint32_t num_targets) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const std::string verb = "uh_pose_mesh";
   HostMesh* mp = nullptr;
   if (int st = posable_mesh(c, mesh_index, verb, &mp)) return st;
   HostMesh& m = *mp;
   if (!m.pose) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": the mesh has neither a skin nor morph targets");
   MeshPose& p = *m.pose;
   if (num_joints != p.num_joints || (num_joints != 0) != (joint_matrices3x4 != nullptr))
      return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": num_joints must be the skin's, with matrices (0 and null without a skin)");
   if (num_targets != p.num_targets || (num_targets != 0) != (morph_weights != nullptr))
      return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": num_targets must be the mesh's, with weights (0 and null without targets)");
   for (size_t i = 0; i < 12 * (size_t)num_joints; i++)
      if (!std::isfinite(joint_matrices3x4[i])) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": a joint matrix is not finite");
   for (uint32_t t = 0; t < num_targets; t++)
      if (!std::isfinite(morph_weights[t])) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": a morph weight is not finite");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   uh_ctx::Pose& u = c->pose;
   for (hipEvent_t& ev : u.ev)
      if (!ev) HIP_TRY(c, hipEventCreate(&ev));
   if (!u.flag.p) HIP_TRY(c, u.flag.alloc(1));
   const uint32_t nv = (uint32_t)m.vertices.size();
   if (!p.back) HIP_TRY(c, hipMalloc((void**)&p.back, nv * sizeof(UhVertex)));
   // the call's parameters in one copy: the matrices, then the active targets as (index, weight) pairs
   std::vector<float>& hp = u.host_params;
   hp.assign(joint_matrices3x4, joint_matrices3x4 + 12 * (size_t)num_joints);
   uint32_t num_active = 0;
   for (uint32_t t = 0; t < num_targets; t++) {
      if (morph_weights[t] == 0.0f) continue;  // the stated rule: a target whose weight is zero is skipped
      float index;
      std::memcpy(&index, &t, sizeof(float));
      hp.push_back(index);
      hp.push_back(morph_weights[t]);
      num_active++;
   }
   if (u.params.n < hp.size()) HIP_TRY(c, u.params.alloc(hp.size()));
   if (!hp.empty()) HIP_TRY(c, hipMemcpyAsync(u.params.p, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemsetAsync(u.flag.p, 0, sizeof(uint32_t), c->stream));
   PoseArgs a;
   a.bind = reinterpret_cast<const float4*>(p.bind);
   a.out = reinterpret_cast<float4*>(p.back);
   a.joints = reinterpret_cast<const uint2*>(p.joints);
   a.weights = reinterpret_cast<const float4*>(p.weights);
   a.mats = reinterpret_cast<const float4*>(u.params.p);
   a.active = reinterpret_cast<const uint2*>(u.params.p + 12 * (size_t)num_joints);  // (48 bytes per joint: 8-byte aligned)
   a.dpos = p.dpos, a.dnrm = p.dnrm;
   a.flag = u.flag.p;
   a.num_vertices = nv, a.num_joints = num_joints, a.num_active = num_active;
   uint32_t flag = 0;
   HIP_TRY(c, hipEventRecord(u.ev[0], c->stream));
   launch_pose(c->stream, a);
   HIP_TRY(c, hipGetLastError());
   HIP_TRY(c, hipEventRecord(u.ev[1], c->stream));
   HIP_TRY(c, hipMemcpyAsync(&flag, u.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   // nothing of the mesh has been touched yet: the pose is in the second buffer
   if (flag) return fail(c, UH_ERR_INVALID_ARGUMENT, verb + ": a posed vertex position is not finite");
   float ms = 0.0f;
   HIP_TRY(c, hipEventElapsedTime(&ms, u.ev[0], u.ev[1]));
   if (int st = replace_mesh_vertices(c, m, "uh_pose_mesh", false, [&]() -> int {
          std::swap(m.d_verts, p.back);  // (a copy instead: 0.04 ms more per million vertices)
          return UH_OK;
       }))
      return st;
   u.st.pose_ms = ms;
   u.st.poses++;
   u.st.vertices = nv;
   u.st.joints = num_joints;
   u.st.active_targets = num_active;
   return UH_OK;
}

int uh_get_pose_stats(uh_ctx* c, UhPoseStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_pose_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (!c->pose.st.poses) return UH_OK;
   *out = c->pose.st;
   out->staged_joint_limit = 0;  // k_pose never stages
   out->device_bytes = c->pose.params.n * sizeof(float) + c->pose.flag.n * sizeof(uint32_t);
   for (const HostMesh& m : c->meshes) {
      if (!m.pose) continue;
      const MeshPose& p = *m.pose;
      const uint64_t nv = m.vertices.size();
      out->device_bytes += nv * sizeof(UhVertex) * (p.back ? 2 : 1) + (p.num_joints ? nv * 24 : 0) + (uint64_t)p.num_targets * nv * (p.dnrm ? 24 : 12);
   }
   return UH_OK;
}

}  // extern "C"
