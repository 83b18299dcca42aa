// hit_shading.h — what one lane does with the hit of its path's ray in a wavefront's shading kernel (reference.rchit:20-92 + rgen:48-61
// and the light-sample selection of rgen:81-110): the body k_shade_hit runs for every bounce and k_primary_shade runs for bounce 0
// (kernels.hip). Both instantiate the same function template, so a path gets the same words from either; the arithmetic itself is
// path_shading.h.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "path_shading.h"

namespace uh {

// per-mesh shading records and texture descriptors of the first kLdsMeshes / kLdsTextures entries: every hit
// gathers 64 + 24 bytes of them per lane, and the kernel is bound by its gather traffic (texture addresser)
constexpr uint32_t kLdsMeshes = 192, kLdsTextures = 64;

// what the kernel around the body holds for it: the tables its block keeps in LDS, and where the paths of this bounce lie and the
// scattered ones go (one shard's segment of the queues, its counters)
struct HitShadeCtx {
   const float* lut;       // LDS: c / 255.0f
   const MeshShade* mesh;  // LDS: the first n_mesh (<= kLdsMeshes) shading records
   const TexInfo* tex;     // LDS: the first n_tex (<= kLdsTextures) texture descriptors
   uint32_t n_mesh, n_tex;
   uint32_t seg;           // first position of the shard's segment
   PathRecs cur, nxt;      // state by position in this bounce's queue / in the next one's
   uint32_t* q_next;       // the next bounce's ray queue (ids; not written with the slim state) and its count
   uint32_t* n_next;
   uint32_t* q_light;      // the bounce's light-ray queue and its count (never touched with the slim state)
   uint32_t* n_light;
};

// one path per lane: `valid` lanes shade their hit; every lane of the wave takes part in the queue appends.
// pos_lit: the path's position in this bounce's queue (without the shard segment); its top bit: the path's sun verdict (kSunLitBit)
// hr: the hit record (t, u, v, packet)
// PRIMARY (bounce must be 0): the caller stands at the path's pixel with the primary ray's state in hand (primary_state's ro / rd): no
// state is read, pos_lit is not used
template <bool SLIM, bool PRIMARY = false>
__device__ __forceinline__ void shade_hit_path(const FrameParams& fp, const SceneDev& sc, const PathState& ps, const HitShadeCtx& cx, uint32_t bounce, uint32_t id,
                                               uint32_t pos_lit, float4 hr, bool valid, float4 primary_o = make_float4(0, 0, 0, 0),
                                               float4 primary_d = make_float4(0, 0, 0, 0)) {
   const uint32_t seg = cx.seg;
   const PathRecs cur = cx.cur, nxt = cx.nxt;
   const uint32_t pos = pos_lit & ~kSunLitBit;
   const bool sun_lit = !PRIMARY && (pos_lit & kSunLitBit) != 0u;
   const uint32_t pk = __float_as_uint(hr.w);
   bool scattered = false, want_light = false;
   uint32_t slot = 0;        // the scattered path's position in the next bounce's queue
   float4 n_o = make_float4(0, 0, 0, 0), n_d = make_float4(0, 0, 0, 0), n_t = make_float4(0, 0, 0, 0), n_r = make_float4(0, 0, 0, 0);  // the scattered path's new state
   if (valid) {
      // every record of the path is requested up front, together with the shading packet (whose index the
      // classification below already read): one round trip for all of them, then one for the texels.
      // The path's state: four planes at its queue position (the RNG words ride in the rays' w components); the lanes of a wave
      // hold hits of nearly consecutive positions, so these are nearly contiguous reads
      float4 ro, rd, thr4;
      if constexpr (PRIMARY) {
         ro = primary_o;
         rd = primary_d;
         thr4 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      } else if (bounce == 0 && fp.primary_implicit) {  // a primary ray's state is not stored (FrameParams::primary_implicit): from its id
         primary_state(fp, id, ro, rd);
         thr4 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      } else {
         ro = ld_rec(rec_quad(cur, seg + pos, REC_ORIGIN));
         rd = ld_rec(rec_quad(cur, seg + pos, REC_DIR));
         thr4 = ld_rec(rec_quad(cur, seg + pos, REC_THR));
      }
      uint2 rng = make_uint2(__float_as_uint(ro.w), __float_as_uint(rd.w));
      if constexpr (SLIM) {
         if (bounce != 0) id = rng.x;  // the origin's w is the path id (at bounce 0 the id came from queue[0], or from the pixel)
         rng.x = 0u;                   // (no raygen RNG word in the slim state: nothing of such a pass reads one)
      }
      float4 rad4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // radiance so far: zero before the first bounce (not materialised)
      if constexpr (!PRIMARY)
         if (rad_stored(fp, bounce)) rad4 = ld_rad<SLIM>(cur, seg + pos, thr4);  // (the compiler waits for it on the spot: measured level with an unconditional read, which costs 16 bytes per hit at bounce 0)
      const V3 ray_dir = v3(rd.x, rd.y, rd.z);
      const float t = hr.x, bu = hr.y, bv = hr.z;
      const float4* sp = sc.shade + 4 * (size_t)pk;  // pk = hr.w, known since the classification: no wait for hr before these
      float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
      const uint32_t mesh_index = __float_as_uint(s3.w);
      // rchit:22-23. The LDS copy is read unconditionally (clamped index, explicit ds_read: device_math.h lds_fetch)
      // and replaced from global memory for the meshes beyond the LDS table
      MeshShade ms = lds_fetch(cx.mesh + (mesh_index < kLdsMeshes ? mesh_index : kLdsMeshes - 1));
      if (mesh_index >= cx.n_mesh) ms = sc.meshes[mesh_index];
      V3 normal;
      float uu, vv;
      surface_normal_uv(s0, s1, s2, s3, bu, bv, normal, uu, vv);                    // rchit:30-31, :39
      // keeps the compiler from sinking the early loads to their first use
      asm volatile("" : "+v"(rng.x), "+v"(rng.y), "+v"(thr4.x), "+v"(thr4.y), "+v"(thr4.z), "+v"(rad4.x), "+v"(rad4.y), "+v"(rad4.z));
      if (sun_lit) rad4 = shadow_lit<false>(thr4, rad4);  // rgen:69-78 of the bounce before: its sun ray left a verdict, the records are here
      const V3 world_normal = world_normal_of(ms, normal, ray_dir);                 // rchit:32-37
      // where the path goes on from (and its sun ray starts): needs nothing the texels bring
      V3 origin = v3(ro.x, ro.y, ro.z) + t * ray_dir;                               // rgen:59
      origin = offset_ray(origin, world_normal);                                    // rgen:60
      // Does the path go on? Decided by the material type and the side the ray came from (rchit:47-89) - nothing the texels
      // bring -, so the scattered paths' places in the next bounce's queue are asked for together with the texels: the returning
      // atomic is in flight with them instead of a round trip of its own after the material evaluation. (Inside the divergent
      // block: the ballot sees the valid lanes, which are the only ones that can scatter.)
      scattered = path_scatters(ms, ray_dir, world_normal);
      const unsigned long long scat_mask = __ballot(scattered);
      const int scat_leader = __ffsll((long long)scat_mask) - 1;
      uint32_t scat_base = 0;
      V3 color = sample_texture_pre(sc, cx.lut, ms.diffuse_map, uu, vv, cx.tex, cx.n_tex, [&] {  // rchit:40
         // (the counter's address goes through a register the compiler cannot see into: for a wave-uniform address its atomic
         // optimiser rewrites the add as a wave reduction with a readfirstlane of the result - and a wait for it - on the spot)
         typedef __attribute__((address_space(1))) uint32_t* global_u32_t;  // (a pointer of unknown address space would make it a flat atomic, which LDS waits wait for)
         global_u32_t counter = (global_u32_t)cx.n_next;
         asm volatile("" : "+v"(counter));
         if (scattered && (int)lane_id() == scat_leader) scat_base = __hip_atomic_fetch_add(counter, (uint32_t)__popcll(scat_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      });
      color = color * v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);    // rchit:41

      uint32_t seed = rng.y;
      const V3 scatter = material_scatter(ms, ray_dir, world_normal, color, seed);  // rchit:47-89
      rng.y = seed;                                                                 // rchit:91
      if (scat_leader >= 0) slot = (uint32_t)__builtin_amdgcn_readlane((int)scat_base, scat_leader) + __builtin_amdgcn_mbcnt_hi((uint32_t)(scat_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)scat_mask, 0u));

      V3 thr = v3(thr4.x, thr4.y, thr4.z) * color;                                  // rgen:48
      if (!scattered) {                                                             // rgen:53-57: the path ends here
         // its radiance goes to the per-id array k_finish_sample reads, with the raygen's RNG word: the next sample of the
         // frame starts from it (rgen:28-31)
         st_stream(ps.radf + id, make_float4(rad4.x + thr.x, rad4.y + thr.y, rad4.z + thr.z, __uint_as_float(rng.x)));
      } else {
         float f = 0.0f;
         int light_index = 0;
         if constexpr (!SLIM)
            if (fp.lights_enabled == 1) want_light = select_light(fp, sc, id, rng.x, origin, f, light_index);  // rgen:81-121
         // the path's state for the next bounce; written below at the position the path gets in the next bounce's queue
         n_o = make_float4(origin.x, origin.y, origin.z, __uint_as_float(SLIM ? id : rng.x));
         n_d = make_float4(scatter.x, scatter.y, scatter.z, __uint_as_float(rng.y));  // rgen:61
         n_t = make_float4(thr.x, thr.y, thr.z, SLIM ? rad4.x : f);
         n_r = make_float4(rad4.x, rad4.y, rad4.z, __uint_as_float((uint32_t)light_index));  // the radiance travels with the path
      }
   }
   // a wave's scattered paths get consecutive positions: their new state leaves as contiguous stores, and the next bounce's
   // traversal, sun-ray and shading kernels read it back as streams
   // the light queue: one round trip - none at all when no lane has an entry
   uint32_t lslot = 0;
   if constexpr (!SLIM) lslot = wave_append(cx.n_light, want_light);
   if (scattered) {
      if constexpr (!SLIM) st_stream(cx.q_next + slot, id);
      st_rec(rec_quad(nxt, seg + slot, REC_ORIGIN), n_o);
      if (bounce + 1 < fp.num_bounces) st_rec(rec_quad(nxt, seg + slot, REC_DIR), n_d);  // (after the last bounce no ray is traced: k_flush_survivors reads radiance and the raygen RNG word)
      st_rec(rec_quad(nxt, seg + slot, REC_THR), n_t);  // (SLIM: w = radiance.r - a zero nobody reads where the radiance is not materialised)
      if (rad_stored(fp, bounce + 1)) {
         if constexpr (SLIM) st_rad_pair(nxt, seg + slot, n_r.y, n_r.z);
         else st_rec(rec_quad(nxt, seg + slot, REC_RAD), n_r);
      }
   }
   if (want_light) st_stream(cx.q_light + lslot, slot);  // the light ray leaves from the path's new position
}

}  // namespace uh
