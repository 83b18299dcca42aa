// path_fused.hip — k_path_fused: bounces 1 .. of a lone frame inside one persistent kernel, and its launcher. The walk is traversal.h's,
// the per-path arithmetic path_shading.h's and the sun grid's look-up grid_walk.h's, all shared with the wavefront's kernels (kernels.hip).
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "grid_walk.h"
#include "kernel_common.h"
#include "path_shading.h"
#include "traversal.h"

namespace uh {

// ------------------------------------------------------------------------------------------
// path_fused - ONE FRAME PER CALL (a moving camera, renderers/mod.rs:357, main.rs:460-471): bounces 1 .. num_bounces - 1 of a lone
// frame inside one persistent kernel. A lone frame's wavefront is some 28 launches of which every traversal launch ends in the tail of
// its longest ray (about 60 dependent steps: 0.30-0.38 ms per bounce for 1.5 M rays against 0.19 ms at the batched rate, DESIGN.md
// section 4) - nothing of the same frame can fill those tails across a launch boundary. Here EVERY BLOCK RUNS ITS OWN WAVEFRONT: a
// block owns a contiguous range of the positions of bounce 1's ray queue (its shard's count / blocks of the shard) and takes those paths
// through all the remaining bounces by itself - trace phase, block barrier, shading phase, block barrier, ... - with no word to any
// other block.
// The paths never move: a path's state stays in its record of set 1 at its position p (shading rewrites it in place), its hit record
// at hit[p]; what a phase hands to the next is a LIST of entries p | flags in the block's range of two of the queue arrays:
//    kHasRay    the path has a ray of the next bounce to trace (its record's origin / direction)
//    kSun       its sun ray was not answered by the grid (border cell, long list - or no grid): the tree's
//    kLight     it asks a light (record: f in throughput.w, light index in radiance.w)
// Trace phase: the block's waves are persistent over the list (the Feeder of the traversal kernels, chunks from a cursor in LDS); a
// lane takes an entry, walks the path's shadow rays first - sun, then light: their results are added to the path's radiance in the
// reference's order (rgen:63-122) -, then its bounce ray, and leaves the hit record. Shadow rays go through the closest-hit walk
// beside the other lanes' bounce rays (occluded <=> the closest hit lies within the limit; the walk stops at the first hit inside).
// Shading phase: k_shade_hit's, over the block's list - hits compacted per wave in LDS and shaded 64 at a time, the sun grid asked on
// the spot; the paths whose ray left the scene gathered per wave too and the sky integrated for 64 of them at a time (reference.rmiss;
// what is left of the list waits in two registers per lane for the next shading phase); ended paths' radiance to the per-id array.
// Bounce 0's sun rays are asked here as well (sun_of_bounce0), so the frame is k_generate, the camera grid, k_shade_hit(0) and
// k_shade_miss(0), this kernel, k_finish_sample.
// Same words per path as the wavefront: the per-path arithmetic is shared (surface_normal_uv .. select_light, make_shadow_ray,
// tri_compute), a path's random numbers depend on nothing but the path, and shadow rays are predicates.
// Round 5 built this kernel four ways, all bit-identical, measured on the same frames (profiles/README.md "One frame per call"): a
// path per LANE (the lane parked at its hit until 32 lanes of the wave stood at one, then the wave shaded them: lane utilisation 0.40,
// 2.6 ms for the four bounces); THIS one (2.29 ms; the wavefront's launches span 2.44); a pipeline per WAVE (hits gathered in LDS and
// shaded 64 at a time between walking steps, the next bounce's rays walked beside this one's stragglers: no drains, lane utilisation
// 0.54 - but a walk's state stays live through the shading: 168 registers, three waves per SIMD, 2.65 ms); a pipeline per BLOCK of
// three walking waves and one shading wave with rings in LDS (101 registers; 2.45-2.54 ms: the shading wave is busy 0.97 of its
// clock). What they show: the walk's rate follows the number of waves that walk - a kernel that also shades has 16, the wavefront's
// traversal kernel 20 to 24 -, and a lone frame's work cannot be had at the batched rate in one kernel. (Two rays per lane in the
// trace phases, both records asked for before either is used: 40 % slower - the walk does not wait for latency.)
// ------------------------------------------------------------------------------------------
constexpr int kFusedBlocks = 4;  // blocks per CU the kernel's registers and LDS are sized for
struct FusedTraceLds {
   uint32_t stack[kWavesPerBlock][kLdsStack][64];
   RayPool<2> pool[kWavesPerBlock];
};
struct FusedShadeLds {
   uint32_t list[kWavesPerBlock][6][128];  // per wave: path ids, positions, the hit record's four words
   uint32_t miss[kWavesPerBlock][2][128];  // per wave: (position, id) of the paths that missed
};
template <bool COUNT, bool INLINE>
__global__ __launch_bounds__(kBlock, kFusedBlocks) void k_path_fused(SceneDev sc, FrameParams fp, PathState ps, Control* ctl, DeviceStats* stats, SunGridDev g, bool use_grid,
                                                                      bool sun_of_bounce0) {
   constexpr uint32_t kFirst = 1;  // the paths are those of bounce 1's ray queue, their state lies in set 1 at their positions there
   // (positions fit 23 bits: the host fuses only when shard_cap < 2^23; bits 23..28: how many bounces follow the entry's ray)
   constexpr uint32_t kHasRay = 1u << 31, kSun = 1u << 30, kLight = 1u << 29, kLeftShift = 23, kLeftMask = 63u << kLeftShift, kPosMask = (1u << kLeftShift) - 1u;
   __shared__ float s_lut[256];
   constexpr uint32_t kLdsMeshes = 128, kLdsTextures = 64;
   __shared__ MeshShade s_mesh[kLdsMeshes];
   __shared__ TexInfo s_tex[kLdsTextures];
   __shared__ union {
      FusedTraceLds t;
      FusedShadeLds s;
   } u;  // the phases alternate
   __shared__ uint32_t s_cursor, s_count[2];
   const uint32_t n_lds_mesh = sc.num_meshes < kLdsMeshes ? sc.num_meshes : kLdsMeshes;
   const uint32_t n_lds_tex = sc.num_textures < kLdsTextures ? sc.num_textures : kLdsTextures;
   s_lut[threadIdx.x] = sc.unorm_lut[threadIdx.x];
   if (threadIdx.x < n_lds_mesh) s_mesh[threadIdx.x] = sc.meshes[threadIdx.x];
   if (threadIdx.x < n_lds_tex) s_tex[threadIdx.x] = sc.textures[threadIdx.x];
   const uint32_t lane = lane_id();
   const uint32_t wave = threadIdx.x >> 6;
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap;
   const PathRecs rec = ps.set[kFirst & 1];
   const uint32_t* __restrict__ ids = ps.queue[kFirst & 1] + seg;  // path id by position
   // the block's range of positions [lo, hi)
   const uint32_t count1 = ctl->q_count[qc_index(kFirst, Q_RAY, sx.shard)];
   const uint32_t per = (((count1 + sx.nb - 1) / sx.nb) + 63u) & ~63u;
   const uint32_t lo = sx.lb * per < count1 ? sx.lb * per : count1, hi = lo + per < count1 ? lo + per : count1;
   uint32_t* lists[2] = {ps.queue[0] + seg + lo, ps.queue[3] + seg + lo};  // at most hi - lo entries each (one per path of the block)
   const uint4* __restrict__ nodes = sc.nodes;
   const float4* __restrict__ tris = sc.tris;
   const V3 sun_d = v3(fp.sun_dir[0], fp.sun_dir[1], fp.sun_dir[2]);
   uint32_t n_nodes = 0, n_tris = 0, n_snodes = 0, n_stris = 0, n_lnodes = 0, n_ltris = 0, n_covered = 0;  // per lane (COUNT only)
   uint32_t w_rays = 0, w_hits = 0, w_sun = 0, w_sun_tree = 0, w_light = 0, w_miss = 0;                      // per wave
   // bounce 1's list: every position of the range, a ray each. sun_of_bounce0: bounce 0's sun rays (rgen:63-79 for the paths
   // k_shade_hit(0) scattered) are asked here instead of by a k_trace_sun_grid / k_trace_shadow pair in front of this kernel - the grid
   // on the spot, what it does not answer as the entry's sun ray in the first trace phase. (Not when lights are on: bounce 0's light
   // rays are the wavefront's, and they come after the sun rays.)
   const uint32_t n_range = hi - lo;
   const uint32_t left1 = (fp.num_bounces - 2u) << kLeftShift;  // bounce 1's rays
   for (uint32_t i0 = 0; i0 < n_range; i0 += kBlock) {
      const uint32_t i = i0 + threadIdx.x;
      const bool valid = i < n_range;
      uint32_t e = (lo + i) | kHasRay | left1;
      bool to_tree = false;
      if (valid && sun_of_bounce0) {
         int r = 2;
         if (use_grid) {
            const float4 ro = ld_rec(rec_quad(rec, seg + lo + i, REC_ORIGIN));
            r = sun_grid_query<COUNT, INLINE>(g, tris, v3(ro.x, ro.y, ro.z), sun_d, n_stris, n_covered);
            if (COUNT) n_snodes++;
         }
         if (r == 0) {  // rgen:69-78
            const float4 t4 = ld_rec(rec_quad(rec, seg + lo + i, REC_THR)), r4 = ld_rec(rec_quad(rec, seg + lo + i, REC_RAD));
            st_rec(rec_quad(rec, seg + lo + i, REC_RAD), make_float4(r4.x + t4.x, r4.y + t4.y, r4.z + t4.z, r4.w));
         }
         if (r == 2) e |= kSun;
         to_tree = r == 2 && use_grid;
      }
      if (valid) lists[0][i] = e;
      if (sun_of_bounce0) {
         w_sun += (uint32_t)__popcll(__ballot(valid));
         w_sun_tree += (uint32_t)__popcll(__ballot(to_tree));
      }
   }
   if (threadIdx.x == 0) {
      s_count[0] = n_range;
      s_count[1] = 0;
      s_cursor = 0;
   }
   __syncthreads();

   // ---- trace phase over lists[which]
   auto trace_phase = [&](uint32_t which) {
      uint32_t* lds_col = &u.t.stack[wave][0][lane];
      RayPool<2>& pool = u.t.pool[wave];
      RaySource src;
      src.queue = lists[which];
      src.count = s_count[which];
      src.cursor = &s_cursor;
      src.wave_index = src.num_waves = 0;
      auto source_of = [&](int a, uint32_t e) { return (const float4*)rec_quad(rec, seg + (e & kPosMask), a == 0 ? REC_ORIGIN : REC_DIR); };
      Feeder<2> f;
      Trav t;
      t.cur = kEmptyRef;
      t.sp = 0;
      enum : uint32_t { BOUNCE_RAY = 0, SUN_RAY = 1, LIGHT_RAY = 2 };
      uint32_t kind = BOUNCE_RAY, entry = 0, rng_x = 0, mark_nodes = 0, mark_tris = 0;
      V3 thr = v3(0, 0, 0), rad = v3(0, 0, 0), scatter = v3(0, 0, 0);
      float lf = 0.0f;
      uint32_t light_bits = 0;
      bool dirty = false;
      uint32_t spill[kSpillStack];
      // the entry's next ray (origin = t.o): sun, light, then the bounce ray - or, behind the last bounce, the path's radiance to the
      // per-id array (what k_flush_survivors writes)
      auto next_ray = [&]() {
         const float4 o4 = make_float4(t.o.x, t.o.y, t.o.z, 0.0f);
         if (entry & kSun) {
            entry &= ~kSun;
            const ShadowRay s = make_shadow_ray<false>(sc, fp, o4, 0u);
            trav_init(t, s.ro, s.rd, s.ro.w, s.rd.w, s.tlimit);
            kind = SUN_RAY;
         } else if (entry & kLight) {
            entry &= ~kLight;
            const ShadowRay s = make_shadow_ray<true>(sc, fp, o4, light_bits);
            trav_init(t, s.ro, s.rd, s.ro.w, s.rd.w, s.tlimit);
            kind = LIGHT_RAY;
         } else {
            const uint32_t p = entry & kPosMask;
            if (entry & kHasRay) {
               if (dirty) st_rec(rec_quad(rec, seg + p, REC_RAD), make_float4(rad.x, rad.y, rad.z, __uint_as_float(light_bits)));
               trav_init(t, o4, make_float4(scatter.x, scatter.y, scatter.z, 0.0f), 0.001f, 10000.0f, INFINITY);  // rgen:61, :45-47
               kind = BOUNCE_RAY;
            } else {  // rgen:127 after the last bounce
               st_stream(ps.radf + ld_stream(ids + p), make_float4(rad.x, rad.y, rad.z, __uint_as_float(rng_x)));
               t.cur = kEmptyRef;
            }
         }
         if (COUNT) {
            mark_nodes = n_nodes;
            mark_tris = n_tris;
         }
      };
      auto take = [&](uint32_t slot) {
         entry = pool.id[slot];
         const float4 ro = pool.v[0][slot], rd = pool.v[1][slot];
         if (entry & (kSun | kLight)) {
            const uint32_t p = entry & kPosMask;
            const float4 t4 = ld_rec(rec_quad(rec, seg + p, REC_THR)), r4 = ld_rec(rec_quad(rec, seg + p, REC_RAD));
            thr = v3(t4.x, t4.y, t4.z);
            lf = t4.w;
            rad = v3(r4.x, r4.y, r4.z);
            light_bits = __float_as_uint(r4.w);
            scatter = v3(rd.x, rd.y, rd.z);
            rng_x = __float_as_uint(ro.w);
            dirty = false;
            t.o = v3(ro.x, ro.y, ro.z);
            next_ray();
         } else {
            trav_init(t, ro, rd, 0.001f, 10000.0f, INFINITY);  // rgen:45-47
            kind = BOUNCE_RAY;
         }
      };
      while (refill_lanes<2>(f, src, pool, t.cur == kEmptyRef, source_of, take)) {
         if (t.cur != kEmptyRef) {
            bool occluded = false;
            bool ended = trav_step<false, COUNT, true>(nodes, tris, t, lds_col, spill, occluded, n_nodes, n_tris);
            // a shadow ray is a predicate: occluded <=> some triangle accepts it within (tmin, tmax) and the light's distance <=> the
            // closest such hit lies within it - the walk can stop at the first hit it finds there (rgen:69, :118-119 read nothing else)
            const bool blocked = t.best.idx != kEmptyRef && t.best.t <= t.tlimit;
            if (kind != BOUNCE_RAY && blocked) ended = true;
            if (ended) {
               if (kind == BOUNCE_RAY) {
                  st_rec(ps.hit + seg + (entry & kPosMask), make_float4(t.best.t, t.best.u, t.best.v, __uint_as_float(t.best.idx)));
                  t.cur = kEmptyRef;
               } else {
                  // rgen:69-78 / :118-122: an unoccluded ray adds the path's throughput (x the light's weight) to its radiance
                  if (!blocked) {
                     rad = kind == SUN_RAY ? v3(rad.x + thr.x, rad.y + thr.y, rad.z + thr.z) : v3(rad.x + thr.x * lf, rad.y + thr.y * lf, rad.z + thr.z * lf);
                     dirty = true;
                  }
                  if (COUNT) {  // the walk's visits belong to the shadow counters
                     const uint32_t dn = n_nodes - mark_nodes, dt = n_tris - mark_tris;
                     n_nodes = mark_nodes;
                     n_tris = mark_tris;
                     if (kind == SUN_RAY) {
                        n_snodes += dn;
                        n_stris += dt;
                     } else {
                        n_lnodes += dn;
                        n_ltris += dt;
                     }
                  }
                  next_ray();  // (t.o is still the point the path's rays leave from)
               }
            }
         }
      }
   };

   uint32_t carry_n = 0, carry_pos = 0, carry_id = 0;
   // ---- shading phase over lists[which] (the entries with a bounce ray: its hit record lies at hit[p]); the scattered paths' entries
   // go to lists[which ^ 1]
   auto shade_phase = [&](uint32_t which) {
      const uint32_t count = s_count[which];
      const uint32_t* __restrict__ cur_list = lists[which];
      uint32_t* nxt_list = lists[which ^ 1];
      uint32_t(*list)[128] = u.s.list[wave];
      uint32_t(*missed)[128] = u.s.miss[wave];
      uint32_t n_list = 0, n_missed = carry_n, n_rays = 0;  // wave-uniform
      if (lane < carry_n) {  // the misses the last shading phase left (fewer than 64: the sky integral runs on full waves)
         missed[0][lane] = carry_pos;
         missed[1][lane] = carry_id;
      }
      __builtin_amdgcn_wave_barrier();
      auto shade = [&](uint32_t id, uint32_t pl, float4 hr, bool valid) {  // pl: the path's position | the bounces left behind this ray
         bool scattered = false, want_light = false, to_tree = false, keep = false;
         uint32_t flags = 0;
         const uint32_t p = pl & kPosMask;
         if (valid) {
            const uint32_t left = (pl & kLeftMask) >> kLeftShift;
            const bool last = left == 0u;
            const uint32_t pk = __float_as_uint(hr.w);
            const float4 ro = ld_rec(rec_quad(rec, seg + p, REC_ORIGIN)), rd = ld_rec(rec_quad(rec, seg + p, REC_DIR)), thr4 = ld_rec(rec_quad(rec, seg + p, REC_THR)),
                         rad4 = ld_rec(rec_quad(rec, seg + p, REC_RAD));
            uint2 rng = make_uint2(__float_as_uint(ro.w), __float_as_uint(rd.w));
            const V3 ray_dir = v3(rd.x, rd.y, rd.z);
            const float4* sp = sc.shade + 4 * (size_t)pk;
            const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
            const uint32_t mesh_index = __float_as_uint(s3.w);
            MeshShade ms = lds_fetch(s_mesh + (mesh_index < kLdsMeshes ? mesh_index : kLdsMeshes - 1));  // rchit:22-23
            if (mesh_index >= n_lds_mesh) ms = sc.meshes[mesh_index];
            V3 normal;
            float uu, vv;
            surface_normal_uv(s0, s1, s2, s3, hr.y, hr.z, normal, uu, vv);                // rchit:30-31, :39
            const V3 world_normal = world_normal_of(ms, normal, ray_dir);                 // rchit:32-37
            V3 origin = v3(ro.x, ro.y, ro.z) + hr.x * ray_dir;                            // rgen:59
            origin = offset_ray(origin, world_normal);                                    // rgen:60
            scattered = path_scatters(ms, ray_dir, world_normal);
            V3 color = sample_texture(sc, s_lut, ms.diffuse_map, uu, vv, s_tex, n_lds_tex);  // rchit:40
            color = color * v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);    // rchit:41
            uint32_t seed = rng.y;
            const V3 scatter = material_scatter(ms, ray_dir, world_normal, color, seed);  // rchit:47-89
            rng.y = seed;                                                                 // rchit:91
            const V3 thr = v3(thr4.x, thr4.y, thr4.z) * color;                            // rgen:48
            V3 rad = v3(rad4.x, rad4.y, rad4.z);
            if (!scattered) {                                                             // rgen:53-57: the path ends here
               st_stream(ps.radf + id, make_float4(rad.x + thr.x, rad.y + thr.y, rad.z + thr.z, __uint_as_float(rng.x)));
            } else {
               float lf = 0.0f;
               int light_index = 0;
               if (fp.lights_enabled == 1) want_light = select_light(fp, sc, id, rng.x, origin, lf, light_index);  // rgen:81-121
               if (fp.sun_shadow_enabled == 1) {                                          // rgen:63-79
                  int r = use_grid ? sun_grid_query<COUNT, INLINE>(g, tris, origin, sun_d, n_stris, n_covered) : 2;
                  if (COUNT && use_grid) n_snodes++;  // every sun ray looked one cell up
                  if (r == 0) rad = v3(rad.x + thr.x, rad.y + thr.y, rad.z + thr.z);       // rgen:69-78
                  if (r == 2) flags |= kSun;
                  to_tree = r == 2 && use_grid;
               }
               if (want_light) flags |= kLight;
               if (!last) flags |= kHasRay | ((left - 1u) << kLeftShift);
               keep = (flags & (kHasRay | kSun | kLight)) != 0u;
               if (!keep) {  // behind the last bounce with no shadow ray out: rgen:127 (what k_flush_survivors writes)
                  st_stream(ps.radf + id, make_float4(rad.x, rad.y, rad.z, __uint_as_float(rng.x)));
               } else {  // the path's state, in place
                  st_rec(rec_quad(rec, seg + p, REC_ORIGIN), make_float4(origin.x, origin.y, origin.z, __uint_as_float(rng.x)));
                  st_rec(rec_quad(rec, seg + p, REC_DIR), make_float4(scatter.x, scatter.y, scatter.z, __uint_as_float(rng.y)));  // rgen:61
                  st_rec(rec_quad(rec, seg + p, REC_THR), make_float4(thr.x, thr.y, thr.z, lf));
                  st_rec(rec_quad(rec, seg + p, REC_RAD), make_float4(rad.x, rad.y, rad.z, __uint_as_float((uint32_t)light_index)));
               }
            }
         }
         const uint32_t slot = wave_append(&s_count[which ^ 1], keep);
         if (keep) nxt_list[slot] = p | flags;
         if (fp.sun_shadow_enabled == 1) w_sun += (uint32_t)__popcll(__ballot(scattered));
         w_sun_tree += (uint32_t)__popcll(__ballot(to_tree));
         w_light += (uint32_t)__popcll(__ballot(want_light));
      };
      // reference.rmiss for `n` paths from the front of the wave's miss list: their state is where shade_miss_path reads it (their
      // records of set 1, untouched since their ray was made)
      auto flush_misses = [&](uint32_t n) {
         if (lane < n) shade_miss_path(fp, ps, seg + missed[0][lane], missed[1][lane], kFirst, false);  // (the kernel adds its sun terms itself)
         w_miss += n;
      };
      auto entry_of = [&](uint32_t k) { return make_float4(__uint_as_float(list[2][k]), __uint_as_float(list[3][k]), __uint_as_float(list[4][k]), __uint_as_float(list[5][k])); };
      const uint32_t rounds = (count + kBlock - 1) / kBlock;
      for (uint32_t r = 0; r < rounds; r++) {
         const uint32_t i = r * kBlock + threadIdx.x;
         uint32_t id = 0, p = 0;
         float4 hr = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kEmptyRef));
         bool has_ray = false;
         if (i < count) {
            const uint32_t e = cur_list[i];
            has_ray = (e & kHasRay) != 0u;  // (an entry without one was a shadow ray behind the last bounce: the trace phase finished it)
            p = e & (kPosMask | kLeftMask);
            if (has_ray) {
               id = ld_stream(ids + (e & kPosMask));
               hr = ld_rec(ps.hit + seg + (e & kPosMask));
            }
         }
         const bool is_hit = __float_as_uint(hr.w) != kEmptyRef;
         const unsigned long long mask = __ballot(is_hit);
         const unsigned long long mmask = __ballot(has_ray && !is_hit);
         n_rays += (uint32_t)__popcll(__ballot(has_ray));
         if (mmask) {
            // reference.rmiss for the paths whose ray left the scene, 64 at a time
            const uint32_t mp = __builtin_amdgcn_mbcnt_hi((uint32_t)(mmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mmask, 0u));
            if (has_ray && !is_hit) {
               missed[0][n_missed + mp] = p & kPosMask;
               missed[1][n_missed + mp] = id;
            }
            n_missed += (uint32_t)__popcll(mmask);
            __builtin_amdgcn_wave_barrier();
            if (n_missed >= 64u) {
               flush_misses(64u);
               const uint32_t rest = n_missed - 64u;
               uint32_t tmp0 = 0, tmp1 = 0;
               if (lane < rest) {
                  tmp0 = missed[0][64u + lane];
                  tmp1 = missed[1][64u + lane];
               }
               __builtin_amdgcn_wave_barrier();
               if (lane < rest) {
                  missed[0][lane] = tmp0;
                  missed[1][lane] = tmp1;
               }
               __builtin_amdgcn_wave_barrier();
               n_missed = rest;
            }
         }
         if (mask == 0ull) continue;
         const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
         if (is_hit) {
            list[0][n_list + prefix] = id;
            list[1][n_list + prefix] = p;
            list[2][n_list + prefix] = __float_as_uint(hr.x);
            list[3][n_list + prefix] = __float_as_uint(hr.y);
            list[4][n_list + prefix] = __float_as_uint(hr.z);
            list[5][n_list + prefix] = __float_as_uint(hr.w);
         }
         n_list += (uint32_t)__popcll(mask);
         __builtin_amdgcn_wave_barrier();
         if (n_list >= 64u) {
            shade(list[0][lane], list[1][lane], entry_of(lane), true);
            w_hits += 64u;
            const uint32_t rest = n_list - 64u;
            uint32_t tmp[6] = {0, 0, 0, 0, 0, 0};
            if (lane < rest)
               for (int k = 0; k < 6; k++) tmp[k] = list[k][64u + lane];
            __builtin_amdgcn_wave_barrier();
            if (lane < rest)
               for (int k = 0; k < 6; k++) list[k][lane] = tmp[k];
            __builtin_amdgcn_wave_barrier();
            n_list = rest;
         }
      }
      if (n_list) {
         shade(lane < n_list ? list[0][lane] : 0u, lane < n_list ? list[1][lane] : 0u, lane < n_list ? entry_of(lane) : make_float4(0.0f, 0.0f, 0.0f, 0.0f), lane < n_list);
         w_hits += n_list;
      }
      // the rest waits in registers for the next shading phase (the list's LDS is the trace phase's stacks)
      carry_n = n_missed;
      if (lane < n_missed) {
         carry_pos = missed[0][lane];
         carry_id = missed[1][lane];
      }
      w_rays += n_rays;
   };

   uint32_t which = 0;
#ifdef UH_FUSED_PROFILE  // (measurement only, with count_visits: the waves' clock in the trace phases / at the barriers / in the shading phases, in the light counters)
   unsigned long long c_trace = 0, c_wait = 0, c_shade = 0;
#define UH_TICK(acc)                                  \
   {                                                  \
      const unsigned long long now = wall_clock64();  \
      acc += now - c_last;                            \
      c_last = now;                                   \
   }
   unsigned long long c_last = wall_clock64();
#else
#define UH_TICK(acc)
#endif
   // phases until a shading phase leaves no entry (every phase takes its entries one bounce on: at most num_bounces + 1 rounds)
   for (uint32_t round_no = 0; round_no < kMaxBounces + 2u; round_no++) {
      if (s_count[which] == 0u && s_count[which ^ 1] == 0u) break;  // (block-uniform: read behind a barrier)
      trace_phase(which);
      UH_TICK(c_trace)
      __syncthreads();  // (workgroup-scope release / acquire: the hit records and radiance the block's waves wrote are visible to all of them)
      UH_TICK(c_wait)
      shade_phase(which);
      UH_TICK(c_shade)
      __syncthreads();
      UH_TICK(c_wait)
      if (threadIdx.x == 0) {
         s_count[which] = 0;
         s_cursor = 0;
      }
      which ^= 1;
      __syncthreads();
   }
   if (carry_n) {  // the last misses: reference.rmiss on a partial wave, once
      if (lane < carry_n) shade_miss_path(fp, ps, seg + carry_pos, carry_id, kFirst, false);
      w_miss += carry_n;
   }
   if (lane == 0) {
      if (w_rays) atomicAdd(&stats->rays[UH_RAY_BOUNCE], (unsigned long long)w_rays);
      if (w_hits) atomicAdd(&stats->closest_hits, (unsigned long long)w_hits);
      if (w_sun) atomicAdd(&stats->rays[UH_RAY_SUN_SHADOW], (unsigned long long)w_sun);
      if (w_sun_tree) atomicAdd(&stats->sun_tree_rays, (unsigned long long)w_sun_tree);
      if (w_light) atomicAdd(&stats->rays[UH_RAY_LIGHT_SHADOW], (unsigned long long)w_light);
      if (w_miss) atomicAdd(&stats->misses, (unsigned long long)w_miss);
   }
   if (COUNT) {
      atomicAdd(&stats->nodes_visited, (unsigned long long)n_nodes);
      atomicAdd(&stats->tris_tested, (unsigned long long)n_tris);
      atomicAdd(&stats->shadow_nodes_visited, (unsigned long long)n_snodes);
      atomicAdd(&stats->shadow_tris_tested, (unsigned long long)n_stris);
      atomicAdd(&stats->light_nodes_visited, (unsigned long long)n_lnodes);
      atomicAdd(&stats->light_tris_tested, (unsigned long long)n_ltris);
      atomicAdd(&stats->sun_covered_rays, (unsigned long long)n_covered);
#ifdef UH_FUSED_PROFILE
      if (lane == 0) {
         atomicAdd(&stats->light_nodes_visited, c_trace);
         atomicAdd(&stats->light_tris_tested, c_wait);
         atomicAdd(&stats->sun_covered_rays, c_shade);
      }
#endif
   }
#undef UH_TICK
}

// bounces 1 .. of a lone frame in one persistent kernel (k_path_fused); g: the sun grid when use_grid
void launch_path_fused(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const PathState& ps, Control* ctl, DeviceStats* stats, const SunGridDev& g,
                       bool use_grid, bool sun_of_bounce0) {
   const dim3 grid = sharded_grid(c.num_cus * c.fused_blocks_per_cu);
   as_constant(c.count_visits, [&](auto count) {
      as_constant(use_grid && g.recs, [&](auto inl) {
         k_path_fused<decltype(count)::value, decltype(inl)::value><<<grid, kBlock, 0, c.stream>>>(sc, fp, ps, ctl, stats, g, use_grid, sun_of_bounce0);
      });
   });
}

}  // namespace uh
