// kernels.hip — gfx950 kernels of the wavefront path tracer.
//
// Replaces (reference, utopian/shaders/): pathtrace_reference/reference.{rgen,rchit,rmiss} and the
// driver's traceRayEXT traversal. One launch of reference.rgen (vkCmdTraceRaysKHR(W,H,1),
// utopian/src/renderers/mod.rs:357) becomes, per sample and bounce, a short chain of launches over
// compacted queues of path ids:
//     generate -> [ trace_closest -> shade_miss | shade_hit -> trace_shadow(sun) -> trace_shadow(light) ]*
//              -> finish_sample
// Bounce 0 of a pass whose primary rays go through the camera grid with nothing stored (SamplePlan::fused_primary, frame_plan.h) is ONE launch,
// k_primary_shade, in place of generate -> trace_camera_grid -> shade_hit(0): primary ray, list walk and hit shading at the pixel.
// Traversal kernels are persistent: a grid that just fills the chip pulls 64-ray batches from a
// device-side cursor until the queue (whose length only the device knows) is drained.
// What other kernel files share with these lives in headers: the BVH4 walk (traversal.h), the per-path shading arithmetic
// (path_shading.h), the body of the hit shading that k_shade_hit and k_primary_shade share (hit_shading.h), the sun grid's look-up (grid_walk.h), grids and block size (kernel_common.h). The lone
// frame's fused kernel is path_fused.hip, the ReSTIR passes restir.hip, the multi-GPU tiles tiles.hip, the hybrid passes hybrid_kernels.hip.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "grid_walk.h"
#include "hit_shading.h"
#include "kernel_common.h"
#include "path_shading.h"
#include "traversal.h"

namespace uh {

// ------------------------------------------------------------------------------------------
// trace_closest — reference.rgen:47 traceRayEXT(..., payload 0) minus the shaders it invokes.
// Reads the bounce's ray queue, writes hit[queue position] = (t, u, v, packet) or packet = kEmptyRef: the shading kernel walks
// the same queue and reads the records back as one contiguous stream (a record per path id was a 64-byte sector per 16-byte
// record there).
// ------------------------------------------------------------------------------------------
// Path rays (sharded): ray_o / ray_d are the origin / direction planes of the bounce's state set, hit_out the hit plane - all by
// queue position, so the rays of a 64-entry chunk are two contiguous kilobytes; their w components carry RNG words: the range is
// rgen:45-47's constants. Raw rays (!sharded, RawRays): record i = ray i, the range is in the w components.
// listed != null (sharded only): the rays are the queue positions listed there (count: Control q_count of kind Q_CAM_TREE) - the
// primary rays k_trace_camera_grid handed over -, already counted.
template <bool COUNT>
__global__ __launch_bounds__(kBlock, 6) void k_trace_closest(SceneDev sc, bool sharded, const float4* __restrict__ ray_o,
                                                               const float4* __restrict__ ray_d, float4* __restrict__ hit_out, uint32_t shard_cap, Control* ctl,
                                                               DeviceStats* stats, uint32_t bounce, uint32_t cursor_slot, int ray_kind, uint32_t raw_count,
                                                               const uint32_t* __restrict__ listed) {
   const bool range_in_w = !sharded;
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   __shared__ RayPool<2> s_pool[kWavesPerBlock];
   const uint32_t lane = lane_id();
   const uint32_t wave = threadIdx.x >> 6;
   uint32_t* lds_col = &s_stack[wave][0][lane];
   RayPool<2>& pool = s_pool[wave];
   RaySource src;
   uint32_t seg = 0;  // first record of this block's rays and results: its shard's segment (path rays) or 0 (raw rays)
   if (sharded) {  // path tracer: this block's shard of the bounce's ray queue, chunks from the shard's cursor; ray = record at its position
      const ShardCtx sx = shard_ctx();
      seg = sx.shard * shard_cap;
      src.queue = listed ? listed + seg : nullptr;
      src.count = ctl->q_count[qc_index(bounce, listed ? Q_CAM_TREE : Q_RAY, sx.shard)];
      src.cursor = &ctl->cursor[cursor_index(cursor_slot, sx.shard)];
      src.wave_index = src.num_waves = 0;
      if (sx.lb == 0 && threadIdx.x == 0) {
         if (!listed) atomicAdd(&stats->rays[ray_kind], (unsigned long long)src.count);
         else if (src.count) atomicAdd(&stats->cam_tree_rays, (unsigned long long)src.count);  // counted as primary rays by the grid kernel already
      }
   } else {
      // stand-alone query over raw_count rays (uh_trace_closest, the G-buffer cast): ray i = record i
      src.queue = nullptr;
      src.count = raw_count;
      src.cursor = nullptr;
      src.wave_index = blockIdx.x * kWavesPerBlock + wave;
      src.num_waves = gridDim.x * kWavesPerBlock;
   }
   const uint4* __restrict__ nodes = sc.nodes;
   const float4* __restrict__ tris = sc.tris;
   auto source_of = [&](int a, uint32_t pos) { return (a == 0 ? ray_o : ray_d) + seg + pos; };
   Feeder<2> f;
   Trav t;
   t.cur = kEmptyRef;
   t.sp = 0;
   uint32_t where = 0, n_nodes = 0, n_tris = 0;
   uint32_t spill[kSpillStack];
   auto take = [&](uint32_t slot) {
      where = seg + (listed ? pool.id[slot] : f.pool_base + slot);  // the ray's position in the queue (the pool holds one chunk: positions pool_base ..)
      const float4 ro = pool.v[0][slot], rd = pool.v[1][slot];
      trav_init(t, ro, rd, range_in_w ? ro.w : 0.001f, range_in_w ? rd.w : 10000.0f, INFINITY);
   };
   while (refill_lanes<2>(f, src, pool, t.cur == kEmptyRef, source_of, take)) {
      if (t.cur != kEmptyRef) {
         bool occluded = false;
         if (trav_step<false, COUNT>(nodes, tris, t, lds_col, spill, occluded, n_nodes, n_tris))
            st_rec(hit_out + where, make_float4(t.best.t, t.best.u, t.best.v, __uint_as_float(t.best.idx)));
      }
   }
   if (COUNT) {
      atomicAdd(&stats->nodes_visited, (unsigned long long)n_nodes);
      atomicAdd(&stats->tris_tested, (unsigned long long)n_tris);
   }
}

// ------------------------------------------------------------------------------------------
// trace_shadow — reference.rgen:67 (sun) and :115 (light): visibility only. The reference runs
// its closest-hit / miss shaders on these rays too, but the raygen reads nothing except
// colorDistance.w (rgen:69,118-119), so the sky integral and material fetch are dead work here.
// Occluded <=> some triangle has tmin < t < tmax (sun) and additionally t <= distance_to_light.
// An unoccluded ray adds its path's throughput (x light weight) to the path's radiance (rgen:69-78 / :118-122).
// ------------------------------------------------------------------------------------------
// leftovers (sun rays only): the rays k_trace_sun_grid could not serve from its grid (queue 3); they are already counted
// VERDICT (sun leftovers only): behind a grid kernel that left verdicts, an unoccluded ray sets its bit in the word the grid kernel
// stored (same stream, so the word is there) - the pool carries the origin alone
// FINAL (with VERDICT; the last bounce of a pass with FrameParams::slim_state): a ray whose walk ends, lit or not, stores its path's
// final radiance - radf[id] = radiance (+ throughput if lit), what k_flush_survivors would have stored - and no verdict; the id is
// the origin's w, throughput and radiance are read where the walk ends (the leftovers are few: no place in the pool for them)
template <bool COUNT, bool LIGHT, bool VERDICT = false, bool FINAL = false>
__global__ __launch_bounds__(kBlock, 5) void k_trace_shadow(SceneDev sc, FrameParams fp, PathState ps, Control* ctl, DeviceStats* stats, uint32_t bounce,
                                                              uint32_t cursor_slot, bool leftovers) {
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   static_assert(!(VERDICT && LIGHT), "verdicts are the sun rays'");
   static_assert(VERDICT || !FINAL, "the final form replaces the verdict");
   constexpr int NA = VERDICT ? 1 : 3;
   __shared__ RayPool<NA> s_pool[kWavesPerBlock];
   const uint32_t lane = lane_id();
   const uint32_t wave = threadIdx.x >> 6;
   uint32_t* lds_col = &s_stack[wave][0][lane];
   RayPool<NA>& pool = s_pool[wave];
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap;
   RaySource src;
   // sun rays leave from every scattered path = every position of the next bounce's ray queue (identity); light rays and the sun
   // rays the grid handed over from the positions listed in their queues
   src.queue = LIGHT ? ps.queue[2] + seg : leftovers ? ps.queue[3] + seg : nullptr;
   src.count = LIGHT ? ctl->q_count[qc_index(bounce, Q_LIGHT, sx.shard)] : leftovers ? ctl->q_count[qc_index(bounce, Q_SUN_TREE, sx.shard)] : ctl->q_count[qc_index(bounce + 1, Q_RAY, sx.shard)];
   src.cursor = &ctl->cursor[cursor_index(cursor_slot, sx.shard)];
   src.wave_index = src.num_waves = 0;
   if (sx.lb == 0 && threadIdx.x == 0) {
      if (!leftovers) atomicAdd(&stats->rays[LIGHT ? UH_RAY_LIGHT_SHADOW : UH_RAY_SUN_SHADOW], (unsigned long long)src.count);
      else if (src.count) atomicAdd(&stats->sun_tree_rays, (unsigned long long)src.count);  // counted as sun rays by the grid kernel already
   }
   const uint4* __restrict__ nodes = sc.nodes;
   const float4* __restrict__ tris = sc.tris;
   const PathRecs rec = ps.set[(bounce + 1) & 1];  // the state of the scattered paths, at their positions in the next bounce's queue
   float4* rad = rec_quad(rec, seg, REC_RAD);
   auto source_of = [&](int a, uint32_t pos) { return (const float4*)rec_quad(rec, seg + pos, a == 0 ? REC_ORIGIN : a == 1 ? REC_THR : REC_RAD); };
   Feeder<NA> f;
   Trav t;
   t.cur = kEmptyRef;
   t.sp = 0;
   uint32_t id = 0, n_nodes = 0, n_tris = 0;  // id: the path's position in the next bounce's queue
   uint32_t path_id = 0;                      // FINAL: the path's id (the slim state's origin.w)
   float4 lit = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   uint32_t spill[kSpillStack];
   auto take = [&](uint32_t slot) {
      id = pool.id[slot];
      ShadowRay s;
      if constexpr (VERDICT) {
         s = make_shadow_ray<false>(sc, fp, pool.v[0][slot], 0u);
         if constexpr (FINAL) path_id = __float_as_uint(pool.v[0][slot].w);
      } else {
         const float4 thr = pool.v[1][slot], r4 = pool.v[2][slot];
         s = make_shadow_ray<LIGHT>(sc, fp, pool.v[0][slot], __float_as_uint(r4.w));
         lit = shadow_lit<LIGHT>(thr, r4);
      }
      trav_init(t, s.ro, s.rd, s.ro.w, s.rd.w, s.tlimit);
   };
   while (refill_lanes<NA>(f, src, pool, t.cur == kEmptyRef, source_of, take)) {
      if (t.cur != kEmptyRef) {
         bool occluded = false;
         const bool ended = trav_step<true, COUNT>(nodes, tris, t, lds_col, spill, occluded, n_nodes, n_tris);
         if constexpr (FINAL) {
            if (ended) {
               const float4 thr = ld_rec(rec_quad(rec, seg + id, REC_THR));
               float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
               if (rad_stored(fp, bounce + 1)) r = ld_rad<true>(rec, seg + id, thr);
               if (!occluded) r = shadow_lit<false>(thr, r);  // rgen:69-78
               st_stream(ps.radf + path_id, make_float4(r.x, r.y, r.z, 0.0f));
            }
         } else if (ended && !occluded) {
            if constexpr (VERDICT)
               atomicOr(sun_lit_word(ps, seg + id), 1ull << (id & 63u));  // no-return: nothing waits for it
            else
               st_stream(rad + id, lit);
         }
      }
   }
   if (COUNT) {
      atomicAdd(LIGHT ? &stats->light_nodes_visited : &stats->shadow_nodes_visited, (unsigned long long)n_nodes);
      atomicAdd(LIGHT ? &stats->light_tris_tested : &stats->shadow_tris_tested, (unsigned long long)n_tris);
   }
}

// ------------------------------------------------------------------------------------------
// trace_sun_grid - the sun shadow rays of reference.rgen:63-79 through the per-direction grid of sun_grid.h instead of the
// tree: one cell look-up, then the cell's packets front (sun side) to back through the same tri_compute<ANY> until one
// occludes the ray or the list falls behind the ray's origin. Same predicate as k_trace_shadow<.., false>: occluded <=> some
// triangle accepts the ray with 0.001 < t < 10000 - bit for bit, the grid only prunes (conservatively) which triangles are asked.
// Batch form: rays do a handful of steps, and their lengths (0..a few tests) differ little inside a wave.
// ------------------------------------------------------------------------------------------
// The lists come in two forms (SunGridDev). Plain: 8-byte entries (packet index, far depth) beside the packet array - two dependent
// reads per test. INLINE: 64-byte records that CARRY their packet (v0 e1 e2 key | this entry's far depth | the next entry's) - one
// sector and one round trip per test; sixty-four bytes per entry where the plain list has eight, so by default only while the records
// stay within four times the packet array (context.hip attach_sun_inline_records, option "sun_grid_inline_max_mb").
// Every position of the next bounce's ray queue is a ray; the coarse cover - when the grid has one - is asked first. (Round 4 also had
// k_shade_hit ask the coarse cover and list the rays it did not answer - level on the frame - and a one-ray-per-lane loop for the plain
// lists: both removed in round 5.)
// VERDICT: the kernel leaves one bit per ray (lit or not) instead of adding the lit rays' throughput to their radiance - see sun_lit_word
// FINAL (with VERDICT; the last bounce of a pass with FrameParams::slim_state): no verdict either - the kernel stands at the surviving
// paths' positions with the verdict in hand, so every ray it does not defer stores its path's final radiance, radf[id] = radiance
// (+ throughput if lit) with the slim state's id, throughput | radiance.r and pair: what k_flush_survivors would have read and stored
template <bool COUNT, bool INLINE, bool VERDICT, bool FINAL = false>
__global__ __launch_bounds__(kBlock) void k_trace_sun_grid(SceneDev sc, FrameParams fp, PathState ps, Control* ctl, DeviceStats* stats, uint32_t bounce,
                                                            uint32_t cursor_slot, SunGridDev g) {
   const uint32_t lane = lane_id();
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap;
   const PathRecs rec = ps.set[(bounce + 1) & 1];  // a sun ray leaves every scattered path: every position of the next bounce's ray queue
   const uint32_t count = ctl->q_count[qc_index(bounce + 1, Q_RAY, sx.shard)];
   uint32_t* cursor = &ctl->cursor[cursor_index(cursor_slot, sx.shard)];
   const V3 d = v3(fp.sun_dir[0], fp.sun_dir[1], fp.sun_dir[2]);  // rgen:64
   uint32_t n_tris = 0, n_covered = 0;
   uint32_t* q_tree = ps.queue[3] + seg;
   uint32_t* n_tree = &ctl->q_count[qc_index(bounce, Q_SUN_TREE, sx.shard)];
   // K rays per lane, each step of the chain (origin -> coarse cover -> cell record -> first list entry [-> its packet] -> throughput /
   // radiance) requested for all K before the first is used: the kernel is a chain of dependent round trips with a few instructions
   // between them, and a wave that keeps K chains in flight hides K times the latency (registers are no constraint: 40 at K = 1)
   constexpr int K = kSunRaysPerLane;
   typedef float f4_t __attribute__((ext_vector_type(4)));  // (arrays of HIP's float4 struct assigned under a condition end up in scratch)
   const f4_t* __restrict__ recs = reinterpret_cast<const f4_t*>(g.recs);       // INLINE
   const f4_t* __restrict__ tris = reinterpret_cast<const f4_t*>(sc.tris);      // plain lists: the packets
   const uint2* __restrict__ entries = reinterpret_cast<const uint2*>(g.entries);
   const uint4* __restrict__ cells = reinterpret_cast<const uint4*>(g.cell_start);  // offset | cover depth | the first entry: packet, far depth
   for (;;) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(cursor, 64u * K);
      base = __builtin_amdgcn_readfirstlane(base);
      if (base >= count) break;
      uint32_t id[K];  // the path's position in the next bounce's queue: its state lies there (a wave reads and writes contiguous kilobytes)
      bool valid[K];
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         id[k] = base + 64u * k + lane;
         valid[k] = id[k] < count;
      });
      float4 ro[K];
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         ro[k] = valid[k] ? ld_rec(rec_quad(rec, seg + id[k], REC_ORIGIN)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      });
      float pw[K];
      uint32_t cx[K], cy[K];
      bool covered[K], ask[K];
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         const V3 o = v3(ro[k].x, ro[k].y, ro[k].z);
         const float pu = dot_fma(v3(g.U[0], g.U[1], g.U[2]), o), pv = dot_fma(v3(g.V[0], g.V[1], g.V[2]), o);
         pw[k] = dot_fma(v3(g.W[0], g.W[1], g.W[2]), o);
         sun_cell_of(g, pu, pv, cx[k], cy[k]);
         covered[k] = false;
      });
      if (g.coarse) {
         float cw[K];
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            cw[k] = valid[k] ? g.coarse[(cy[k] >> g.coarse_shift) * g.coarse_nx + (cx[k] >> g.coarse_shift)] : -INFINITY;
         });
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            covered[k] = valid[k] && sun_coarse_covered(cw[k], pw[k]);
         });
      }
      uint4 cs[K];  // offset into the entries | cover depth | first entry: packet | far depth
      uint32_t end[K];
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         ask[k] = valid[k] && !covered[k];
         cs[k] = make_uint4(0u, 0u, 0u, 0u);
         end[k] = 0u;
         if (ask[k]) {
            const uint32_t cell = cy[k] * g.nx + cx[k];
            cs[k] = cells[cell];
            end[k] = cells[cell + 1].x;
         }
      });
      bool defer[K], walk[K], lit[K];
      f4_t ra[K], rb[K], rc[K];  // the first packet; INLINE: rc.z / rc.w = this entry's far depth / the next one's
      uint2 en[K], nxt[K];       // plain lists: this entry (packet, far depth) and the next
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         // the cell's cover: some packet spans the whole cell (with the margins to spare) and every ray that starts below this depth has
         // it in front, further than tmin away and nearer than tmax (sun_grid.h kSunCoverReach) - occluded, as the tree walk would say
         const float cover = __uint_as_float(cs[k].y);
         const bool cov = ask[k] && pw[k] < cover && cover - pw[k] < kSunCoverReach;
         covered[k] = covered[k] || cov;
         // a border cell stands for everything beyond the dense part of the scene, and some interior cells list a great many packets
         // (walls edge-on to the sun): such a ray is cheaper in the tree - k_trace_shadow takes it from queue 3
         defer[k] = ask[k] && !cov && (cx[k] == 0 || cy[k] == 0 || cx[k] + 1 == g.nx || cy[k] + 1 == g.ny || end[k] - cs[k].x > g.max_walk);
         walk[k] = ask[k] && !cov && !defer[k] && cs[k].x < end[k];
         lit[k] = ask[k] && !cov && !defer[k] && !walk[k];  // nothing projects into the cell
         if (walk[k]) {
            if constexpr (INLINE) {
               const f4_t* r = recs + 4 * (size_t)cs[k].x;
               ra[k] = r[0];
               rb[k] = r[1];
               rc[k] = r[2];
            } else {
               // the list's first entry came with the cell record: its packet is asked for at once, the second entry beside it
               en[k] = make_uint2(cs[k].z, cs[k].w);
               // sorted by far depth, descending: a list whose first entry ends behind the origin has nothing in front of the ray
               if (__uint_as_float(en[k].y) < pw[k]) {
                  walk[k] = false;
                  lit[k] = true;
               } else {
                  const f4_t* r = tris + kTriStride16 * (size_t)en[k].x;
                  ra[k] = r[0];
                  rb[k] = r[1];
                  rc[k] = r[2];
                  nxt[k] = cs[k].x + 1 < end[k] ? entries[cs[k].x + 1] : make_uint2(0u, 0u);
               }
            }
         }
         if (COUNT) n_covered += covered[k] ? 1u : 0u;
      });
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         if (walk[k]) {
            const V3 o = v3(ro[k].x, ro[k].y, ro[k].z);
            Hit best;
            best.t = 10000.0f;  // tmax (rgen:66)
            best.u = best.v = 0.0f;
            best.idx = kEmptyRef;
            best.key = 0xffffffffu;
            uint32_t e = cs[k].x;
            float4 a = make_float4(ra[k].x, ra[k].y, ra[k].z, ra[k].w), b = make_float4(rb[k].x, rb[k].y, rb[k].z, rb[k].w), c = make_float4(rc[k].x, rc[k].y, rc[k].z, rc[k].w);
            bool occluded = false;
            if constexpr (INLINE) {
               const f4_t* r = recs + 4 * (size_t)e;
               for (;;) {
                  if (c.z < pw[k]) break;  // from here on every packet ends behind the origin (t < 0 for all of them)
                  if (COUNT) n_tris++;
                  if (tri_compute<true>(a, b, c, 0u, o, d, 0.001f, INFINITY, best)) {
                     occluded = true;
                     break;
                  }
                  e++;
                  if (e >= end[k] || c.w < pw[k]) break;  // the next record is only asked for when the ray has to go on
                  r += 4;
                  const f4_t na = r[0], nb = r[1], nc = r[2];
                  a = make_float4(na.x, na.y, na.z, na.w);
                  b = make_float4(nb.x, nb.y, nb.z, nb.w);
                  c = make_float4(nc.x, nc.y, nc.z, nc.w);
               }
            } else {
               uint2 cur = en[k], nx = nxt[k];
               for (;;) {
                  if (COUNT) n_tris++;
                  if (tri_compute<true>(a, b, c, cur.x, o, d, 0.001f, INFINITY, best)) {
                     occluded = true;
                     break;
                  }
                  e++;
                  if (e >= end[k] || __uint_as_float(nx.y) < pw[k]) break;
                  cur = nx;
                  if (e + 1 < end[k]) nx = entries[e + 1];  // in flight with the packet
                  const f4_t* r = tris + kTriStride16 * (size_t)cur.x;
                  const f4_t na = r[0], nb = r[1], nc = r[2];
                  a = make_float4(na.x, na.y, na.z, na.w);
                  b = make_float4(nb.x, nb.y, nb.z, nb.w);
                  c = make_float4(nc.x, nc.y, nc.z, nc.w);
               }
            }
            lit[k] = !occluded;
         }
      });
      if constexpr (FINAL) {
         static_assert(VERDICT, "the final form replaces the verdict");
         const bool stored = rad_stored(fp, bounce + 1);
         float4 thr[K], rad[K];
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            rad[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (valid[k] && !defer[k]) {
               thr[k] = ld_rec(rec_quad(rec, seg + id[k], REC_THR));
               if (stored) rad[k] = ld_rad<true>(rec, seg + id[k], thr[k]);
            }
         });
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (valid[k] && !defer[k]) {
               if (lit[k]) rad[k] = shadow_lit<false>(thr[k], rad[k]);  // rgen:69-78: radiance += throughput
               st_stream(ps.radf + __float_as_uint(ro[k].w), make_float4(rad[k].x, rad[k].y, rad[k].z, 0.0f));
            }
         });
      } else if constexpr (VERDICT) {
         // lane l of sub-chunk k holds position base + 64 k + l (the cursor starts at 0 and moves by 64 K; segments start at multiples
         // of 64): the ballot is that run's verdict word. Deferred rays and lanes beyond the count contribute 0 - the leftover kernel
         // sets the bits of the deferred rays it finds lit. Every word below the count is stored, so the plane needs no clearing.
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const unsigned long long word = __ballot(lit[k]);
            if (lane == 0 && base + 64u * k < count) *sun_lit_word(ps, seg + base + 64u * k) = word;
         });
      } else {
         float4 thr[K], rad[K];
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (lit[k]) {  // rgen:69-78: radiance += throughput
               thr[k] = ld_rec(rec_quad(rec, seg + id[k], REC_THR));
               rad[k] = ld_rec(rec_quad(rec, seg + id[k], REC_RAD));
            }
         });
         static_for<K>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (lit[k]) st_rec(rec_quad(rec, seg + id[k], REC_RAD), shadow_lit<false>(thr[k], rad[k]));
         });
      }
      static_for<K>([&](auto kc) {
         constexpr int k = decltype(kc)::value;
         if (__ballot(defer[k]) != 0ull) {  // wave-uniform: every lane of the wave takes part in the append
            const uint32_t slot = wave_append(n_tree, defer[k]);
            if (defer[k]) st_stream(q_tree + slot, id[k]);
         }
      });
   }
   if (sx.lb == 0 && threadIdx.x == 0) {
      atomicAdd(&stats->rays[UH_RAY_SUN_SHADOW], (unsigned long long)count);
      if (COUNT) atomicAdd(&stats->shadow_nodes_visited, (unsigned long long)count);  // every sun ray looked one cell (or its block's coarse cover) up
   }
   if (COUNT) {
      atomicAdd(&stats->shadow_tris_tested, (unsigned long long)n_tris);
      atomicAdd(&stats->sun_covered_rays, (unsigned long long)n_covered);
   }
}

// ------------------------------------------------------------------------------------------
// trace_camera_grid - the primary rays of reference.rgen:31-47 (bounce 0 of the path tracer) through the per-camera grid of
// sun_grid.h "camera grid" instead of the tree: the ray's cell is its own pixel, the cell's packets are tested front to back
// with the closest-hit test of the tree walk (tri_compute<false>: the same t, u, v and the same tie-break by key) until the next
// packet's distance bound exceeds the best hit. Same hit record as k_trace_closest, bit for bit: the grid only prunes
// (conservatively) which triangles are asked. A pixel whose list is longer than max_walk hands its ray to the tree walk
// (queue 3, Q_CAM_TREE: k_trace_closest over the listed positions, right after this kernel).
// The 64 rays of a wave are 64 neighbouring pixels: cell records, entries and packets are shared or adjacent - this kernel runs
// out of the caches where the tree walk of the same rays fetched ~20 records per ray.
// ------------------------------------------------------------------------------------------
// the walk of one pixel's list [e, end) by its primary ray (k_trace_camera_grid, k_primary_shade): the closest hit among the list's packets,
// idx = kEmptyRef for none. sorted: the builder sorted the list by the distance bound, the walk ends where the bound passes the best hit;
// otherwise (a list longer than max_walk, walked whole under walk_whole) every packet is tested.
template <bool COUNT>
__device__ __forceinline__ Hit camera_list_walk(const SunGridDev& g, const float4* __restrict__ tris, uint32_t e, uint32_t end, bool sorted, V3 o, V3 d, uint32_t& n_tris) {
   Hit best;
   best.t = 10000.0f;  // rgen:45: tmax
   best.u = best.v = 0.0f;
   best.idx = kEmptyRef;
   best.key = 0xffffffffu;
   uint2 en = make_uint2(0u, 0u);
   if (e < end) en = reinterpret_cast<const uint2*>(g.entries)[e];
   while (e < end) {
      // sorted by the bound, ascending: from here on no packet can be hit nearer than the best hit (nor tie with it)
      if (sorted && -__uint_as_float(en.y) > best.t) break;
      const uint32_t pk = en.x;
      uint2 nxt = make_uint2(0u, 0u);
      if (e + 1 < end) nxt = reinterpret_cast<const uint2*>(g.entries)[e + 1];  // in flight with the packet
      const float4 a = tris[kTriStride16 * (size_t)pk + 0], b = tris[kTriStride16 * (size_t)pk + 1], c = tris[kTriStride16 * (size_t)pk + 2];
      if (COUNT) n_tris++;
      tri_compute<false>(a, b, c, pk, o, d, 0.001f, INFINITY, best);
      en = nxt;
      e++;
   }
   return best;
}

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void k_trace_camera_grid(SceneDev sc, FrameParams fp, PathState ps, Control* ctl, DeviceStats* stats, uint32_t cursor_slot, SunGridDev g) {
   const uint32_t lane = lane_id();
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap;
   const uint32_t* __restrict__ queue = ps.queue[0] + seg;
   const uint32_t count = ctl->q_count[qc_index(0, Q_RAY, sx.shard)];
   uint32_t* cursor = &ctl->cursor[cursor_index(cursor_slot, sx.shard)];
   const PathRecs rec = ps.set[0];
   const float4* __restrict__ tris = sc.tris;
   uint32_t* q_tree = ps.queue[3] + seg;
   uint32_t* n_tree = &ctl->q_count[qc_index(0, Q_CAM_TREE, sx.shard)];
   uint32_t n_tris = 0;
   for (;;) {
      const uint32_t base = next_batch(cursor);
      if (base >= count) break;
      const uint32_t i = base + lane;
      const bool valid = i < count;
      bool defer = false;
      if (valid) {
         const uint32_t id = ld_stream(queue + i);
         const uint32_t k = id % fp.n_owned;
         const uint32_t pix = fp.owned_pixels ? fp.owned_pixels[k] : k;
         const uint32_t px = pix % fp.W, py = pix / fp.W;
         const uint32_t cell = (py + 1) * g.nx + (px + 1);
         uint32_t e = g.cell_start[cell];  // the camera grid's cell records are plain offsets (no cover depths)
         const uint32_t end = g.cell_start[cell + 1];
         const bool sorted = end - e <= g.max_walk;  // the builder sorts the lists a ray may walk with the early exit
         defer = end - e > (g.walk_whole > g.max_walk ? g.walk_whole : g.max_walk);
         if (defer && fp.primary_implicit) {  // the tree walk reads its rays from the planes: this one's is written after all
            float4 ro, rd;
            primary_state(fp, id, ro, rd);
            st_rec(rec_quad(rec, seg + i, REC_ORIGIN), ro);
            st_rec(rec_quad(rec, seg + i, REC_DIR), rd);
         }
         if (!defer) {
            float4 ro, rd;
            if (fp.primary_implicit)
               primary_state(fp, id, ro, rd);
            else {
               ro = ld_rec(rec_quad(rec, seg + i, REC_ORIGIN));
               rd = ld_rec(rec_quad(rec, seg + i, REC_DIR));
            }
            const Hit best = camera_list_walk<COUNT>(g, tris, e, end, sorted, v3(ro.x, ro.y, ro.z), v3(rd.x, rd.y, rd.z), n_tris);
            st_rec(ps.hit + seg + i, make_float4(best.t, best.u, best.v, __uint_as_float(best.idx)));
         }
      }
      if (__ballot(defer) != 0ull) {  // wave-uniform: every lane of the wave takes part in the append
         const uint32_t slot = wave_append(n_tree, defer);
         if (defer) st_stream(q_tree + slot, i);
      }
   }
   if (sx.lb == 0 && threadIdx.x == 0) atomicAdd(&stats->rays[UH_RAY_PRIMARY], (unsigned long long)count);
   if (COUNT) atomicAdd(&stats->cam_tris_tested, (unsigned long long)n_tris);
}

// the G-buffer cast (gbuffer.rs:11-52 as a primary-ray cast: k_gbuffer_generate) through the camera grid: ray j of the cast is the ray
// through the centre of pixel spans.pixel_of(j). A pixel whose list is too long to have been sorted is walked whole (no early exit).
__global__ __launch_bounds__(kBlock) void k_gbuffer_camera_grid(SceneDev sc, RawRays ps, RowSpans spans, uint32_t W, SunGridDev g) {
   const uint32_t n = spans.total();
   const float4* __restrict__ tris = sc.tris;
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
      const uint32_t pix = spans.pixel_of(j);
      const uint32_t px = pix % W, py = pix / W;
      const uint32_t cell = (py + 1) * g.nx + (px + 1);
      uint32_t e = g.cell_start[cell];
      const uint32_t end = g.cell_start[cell + 1];
      const bool sorted = end - e <= g.max_walk;
      const float4 ro = ps.ray_o[j], rd = ps.ray_d[j];
      const V3 o = v3(ro.x, ro.y, ro.z), d = v3(rd.x, rd.y, rd.z);
      Hit best;
      best.t = rd.w;
      best.u = best.v = 0.0f;
      best.idx = kEmptyRef;
      best.key = 0xffffffffu;
      for (; e < end; e++) {
         const uint2 en = reinterpret_cast<const uint2*>(g.entries)[e];
         if (sorted && -__uint_as_float(en.y) > best.t) break;
         const uint32_t pk = en.x;
         const float4 a = tris[kTriStride16 * (size_t)pk + 0], b = tris[kTriStride16 * (size_t)pk + 1], c = tris[kTriStride16 * (size_t)pk + 2];
         tri_compute<false>(a, b, c, pk, o, d, ro.w, INFINITY, best);
      }
      ps.hit[j] = make_float4(best.t, best.u, best.v, __uint_as_float(best.idx));
   }
}

// stand-alone any-hit query (uh_trace_any): occluded[i] = 1 when some triangle lies in (tmin, tmax) of ray i
__global__ __launch_bounds__(kBlock) void k_trace_any_raw(SceneDev sc, const float4* __restrict__ ray_o, const float4* __restrict__ ray_d,
                                                          uint32_t* __restrict__ occluded, uint32_t count) {
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   uint32_t* lds_col = &s_stack[threadIdx.x >> 6][0][lane_id()];
   uint32_t n_nodes = 0, n_tris = 0;
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
      float4 ro = ray_o[i], rd = ray_d[i];
      Hit h;
      occluded[i] = traverse<true, false>(sc, v3(ro.x, ro.y, ro.z), v3(rd.x, rd.y, rd.z), ro.w, rd.w, INFINITY, h, lds_col, n_nodes, n_tris) ? 1u : 0u;
   }
}

// ------------------------------------------------------------------------------------------
// generate — reference.rgen:24-40: RNG init, payload seed copy, jitter, primary ray
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_generate(FrameParams fp, PathState ps, Control* ctl, uint32_t sample) {
   const uint32_t n = fp.n_owned * fp.batch_frames;  // owned pixels x frames of the batch
   const uint32_t lane = lane_id();
   const uint32_t groups = (n + 63) / 64;
   // one wave per 64 owned pixels; a path's shard (shard_of_run of its 64-path run) decides which queue segment receives its id,
   // and its state goes to the position it gets there (set 0: the state of bounce 0's queue) - the 64 paths of a wave are one
   // run, so one append hands them 64 consecutive positions: plain coalesced 1-KiB stores per plane
   for (uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += gridDim.x * kWavesPerBlock) {
      const uint32_t q = g * 64u + lane;
      bool own = q < n;
      uint32_t id = 0;
      float4 s_o = make_float4(0, 0, 0, 0), s_d = make_float4(0, 0, 0, 0);
      if (own) id = q;
      if (own && !fp.primary_implicit) {  // (primary_implicit: the kernels of bounce 0 compute the state from the id)
         // path id = frame of the batch x owned pixels + index into the rank's owned-pixel list: dense, so a rank's wavefront
         // carries as many frames as its share of the frame allows (on one GPU: frame x W x H + pixel)
         const uint32_t f = q / fp.n_owned, k = q - f * fp.n_owned;
         const uint32_t pix = fp.owned_pixels ? fp.owned_pixels[k] : k;
         uint32_t px = pix % fp.W, py = pix / fp.W;
         uint32_t rng = sample == 0 ? init_rng(px, py, fp.W, fp.frame_numbers[f]) : __float_as_uint(ps.radf[id].w);  // rgen:24; later samples: where the last one left it
         uint32_t seed = rng;                                                                   // rgen:30
         float jx = random_float(rng), jy = random_float(rng);                                  // rgen:31
         V3 o, d;
         primary_ray(fp, px, py, jx, jy, o, d);
         s_o = make_float4(o.x, o.y, o.z, __uint_as_float(fp.slim_state ? id : rng));  // (slim state: the path id rides with the origin in every set)
         s_d = make_float4(d.x, d.y, d.z, __uint_as_float(seed));
         // radiance = 0 / pixelColor = 0 (rgen:26,40) are not materialised: the bounce-0 shading kernels and the first
         // finish_sample use the constants directly
      }
      // the 64 paths of a wave are one run of ids (hence one shard); the loop below is kept for the general case
      uint32_t shard = own ? shard_of_run(id >> 6) : 0xffffffffu;
      unsigned long long todo = __ballot(own);
      while (todo) {
         const int leader = __ffsll((long long)todo) - 1;
         const uint32_t s = __shfl(shard, leader);
         const bool mine = own && shard == s;
         uint32_t slot = wave_append(&ctl->q_count[qc_index(0, Q_RAY, s)], mine);
         if (mine) {
            const uint32_t pos = s * ps.shard_cap + slot;
            ps.queue[0][pos] = id;
            if (!fp.primary_implicit) {
               st_rec(rec_quad(ps.set[0], pos, REC_ORIGIN), s_o);
               st_rec(rec_quad(ps.set[0], pos, REC_DIR), s_d);
               st_rec(rec_quad(ps.set[0], pos, REC_THR), make_float4(1.0f, 1.0f, 1.0f, 0.0f));  // throughput = 1 (rgen:39)
            }
         }
         todo &= ~__ballot(mine);
      }
   }
}

// ------------------------------------------------------------------------------------------
// shade_miss — reference.rmiss:10-31 + rgen:48-57 for paths whose ray left the scene.
// Walks the bounce's RAY queue and picks out the paths whose hit record says "miss" (the traversal
// kernels build no hit / miss queues). The sky integral is ~3k VALU instructions per path, so the
// misses are first compacted inside the wave: ids collect in a per-wave LDS list and the integral
// runs on 64 of them at a time with every lane live.
// ------------------------------------------------------------------------------------------
// The bounce's misses arrive as a queue of their own (Q_MISS), written by k_shade_hit while it classifies the bounce's RAY
// queue: every lane has a path, no hit record is read here, and nothing but the sky integral (~600 VALU instructions per
// path) and four 16-byte records per path is left in the kernel. The position's top bit is the path's sun verdict (kSunLitBit).
// SLIM (FrameParams::slim_state): behind bounce 0 the entry's id word is not one - the id is in the origin quad (shade_miss_path)
template <bool SLIM>
__global__ __launch_bounds__(kBlock) void k_shade_miss(FrameParams fp, PathState ps, Control* ctl, DeviceStats* stats, uint32_t bounce) {
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap;
   const uint2* __restrict__ queue = reinterpret_cast<const uint2*>(ps.queue[4]) + seg;  // (position in the bounce's ray queue, path id)
   const uint32_t count = ctl->q_count[qc_index(bounce, Q_MISS, sx.shard)];
   for (uint32_t i = sx.lb * kBlock + threadIdx.x; i < count; i += sx.nb * kBlock) {
      const uint2 e = ld_stream(queue + i);
      shade_miss_path<SLIM>(fp, ps, seg + (e.x & ~kSunLitBit), e.y, bounce, (e.x & kSunLitBit) != 0u);
   }
   if (sx.lb == 0 && threadIdx.x == 0 && count) atomicAdd(&stats->misses, (unsigned long long)count);
}

// ------------------------------------------------------------------------------------------
// shade_hit — reference.rchit:20-92 + rgen:48-61 and the light-sample selection of rgen:81-110
// ------------------------------------------------------------------------------------------
// SLIM (FrameParams::slim_state; device_types.h PathState): the path id arrives with the origin quad and leaves with it - behind bounce 0
// no id is loaded from queue[b & 1], and none is appended to the next queue at any bounce: the queue is its count, the state planes by
// position are its content. Radiance: r beside the throughput, (g, b) as a pair. No light sample (the pass has no lights).
template <bool SLIM>
__global__ __launch_bounds__(kBlock, kShadeHitBlocks) void k_shade_hit(FrameParams fp, SceneDev sc, PathState ps, Control* ctl, DeviceStats* stats, uint32_t bounce) {
   // c / 255.0f table in LDS: the 12 per-fetch table gathers were texture-addresser traffic (the
   // kernel ran 86 % TA-busy at 2 % VALU, profiles/r01c_*); LDS serves them at no TA cost
   __shared__ float s_lut[256];
   s_lut[threadIdx.x] = sc.unorm_lut[threadIdx.x];
   // the first kLdsMeshes / kLdsTextures per-mesh shading records and texture descriptors (hit_shading.h)
   __shared__ MeshShade s_mesh[kLdsMeshes];
   __shared__ TexInfo s_tex[kLdsTextures];
   const uint32_t n_lds_mesh = sc.num_meshes < kLdsMeshes ? sc.num_meshes : kLdsMeshes;
   const uint32_t n_lds_tex = sc.num_textures < kLdsTextures ? sc.num_textures : kLdsTextures;
   __shared__ uint32_t s_hits;
   __shared__ uint32_t s_list[kWavesPerBlock][6][128];  // per wave: path ids, their queue positions, and the hit record (t, u, v, packet) the classification read with them
   __shared__ uint32_t s_miss[kWavesPerBlock][2][128];  // per wave: (position, id) of the paths that missed, handed to k_shade_miss 64 at a time
   if (threadIdx.x == 0) s_hits = 0;
   if (threadIdx.x < n_lds_mesh) s_mesh[threadIdx.x] = sc.meshes[threadIdx.x];
   if (threadIdx.x < n_lds_tex) s_tex[threadIdx.x] = sc.textures[threadIdx.x];
   __syncthreads();
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap;
   // the bounce's RAY queue: paths whose hit record says "miss" belong to k_shade_miss and are skipped here
   const uint32_t count = ctl->q_count[qc_index(bounce, Q_RAY, sx.shard)];
   const uint32_t* __restrict__ queue = ps.queue[bounce & 1] + seg;
   const PathRecs cur = ps.set[bounce & 1], nxt = ps.set[(bounce + 1) & 1];  // state by position in this bounce's queue / in the next one's
   uint32_t* q_next = ps.queue[(bounce + 1) & 1] + seg;
   uint32_t* n_next = &ctl->q_count[qc_index(bounce + 1, Q_RAY, sx.shard)];
   uint32_t* q_light = ps.queue[2] + seg;
   uint32_t* n_light = &ctl->q_count[qc_index(bounce, Q_LIGHT, sx.shard)];
   uint2* q_miss = reinterpret_cast<uint2*>(ps.queue[4]) + seg;
   uint32_t* n_miss = &ctl->q_count[qc_index(bounce, Q_MISS, sx.shard)];
   const uint32_t stride = sx.nb * kBlock;
   const uint32_t rounds = (count + stride - 1) / stride;
   uint32_t n_hits = 0;
   // one path per lane (hit_shading.h shade_hit_path: the body k_primary_shade shares): `valid` lanes shade their hit; every lane of the
   // wave takes part in the queue appends. pos_lit: the position in this bounce's queue (without the shard segment) | kSunLitBit
   const HitShadeCtx hx{s_lut, s_mesh, s_tex, n_lds_mesh, n_lds_tex, seg, cur, nxt, q_next, n_next, q_light, n_light};
   auto shade = [&](uint32_t id, uint32_t pos_lit, float4 hr, bool valid) { shade_hit_path<SLIM>(fp, sc, ps, hx, bounce, id, pos_lit, hr, valid); };
   // The bounce's RAY queue holds hits and misses (the traversal kernels build no hit / miss queues). Shading a wave of
   // queue entries as they come leaves the lanes of the misses idle through the whole material evaluation, so the hits
   // are first compacted inside the wave: their ids collect in a per-wave LDS list and are shaded 64 at a time.
   uint32_t(*list)[128] = s_list[threadIdx.x >> 6];  // [0] ids, [1] positions, [2..5] the hit record's four words
   uint32_t(*missed)[128] = s_miss[threadIdx.x >> 6];  // [0] positions, [1] ids
   const uint32_t lane = lane_id();
   uint32_t n_list = 0, n_missed = 0;  // wave-uniform
   // the sun rays of the bounce before left verdicts, one bit per position of this queue: a wave's 64 entries are one aligned word
   const bool verdicts = bounce != 0 && fp.sun_verdicts != 0;
   // `n` entries from the front of the wave's miss list go to the bounce's miss queue (one atomic per call)
   auto flush_misses = [&](uint32_t n) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(n_miss, n);
      base = __shfl(base, 0);
      if (lane < n) st_stream(q_miss + base + lane, make_uint2(missed[0][lane], missed[1][lane]));
   };
   auto entry = [&](uint32_t k) { return make_float4(__uint_as_float(list[2][k]), __uint_as_float(list[3][k]), __uint_as_float(list[4][k]), __uint_as_float(list[5][k])); };
   for (uint32_t r = 0; r < rounds; r++) {
      const uint32_t i = r * stride + sx.lb * kBlock + threadIdx.x;
      uint32_t id = 0;
      float4 hr = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kEmptyRef));
      if (i < count) {
         if (!SLIM || bounce == 0) id = ld_stream(queue + i);  // (SLIM behind bounce 0: the id comes with the origin quad; the lists' id words are unused)
         // the whole record (one 16-byte lane load, as the packet index alone would be): shade() does not read it again. The
         // traversal kernel left it at the ray's queue position: the wave reads 1 KiB in one piece
         hr = ld_rec(ps.hit + seg + i);
      }
      uint32_t i_lit = i;  // the position with the path's verdict beside it
      if (verdicts) {
         const uint32_t i0 = __builtin_amdgcn_readfirstlane(i - lane);  // wave-uniform: one load for the wave
         if (i0 < count && ((*sun_lit_word(ps, seg + i0) >> lane) & 1ull)) i_lit |= kSunLitBit;
      }
      const bool is_hit = __float_as_uint(hr.w) != kEmptyRef;
      const unsigned long long mask = __ballot(is_hit);
      const unsigned long long mmask = __ballot(i < count && !is_hit);
      if (mmask) {
         const uint32_t mp = __builtin_amdgcn_mbcnt_hi((uint32_t)(mmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mmask, 0u));
         if (i < count && !is_hit) {
            missed[0][n_missed + mp] = i_lit;
            missed[1][n_missed + mp] = id;
         }
         n_missed += (uint32_t)__popcll(mmask);
         __builtin_amdgcn_wave_barrier();
         if (n_missed >= 64u) {
            flush_misses(64u);
            const uint32_t rest = n_missed - 64u;  // at most 63: to the front (one wave, LDS operations execute in order)
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
         if (!SLIM || bounce == 0) list[0][n_list + prefix] = id;
         list[1][n_list + prefix] = i_lit;
         list[2][n_list + prefix] = __float_as_uint(hr.x);
         list[3][n_list + prefix] = __float_as_uint(hr.y);
         list[4][n_list + prefix] = __float_as_uint(hr.z);
         list[5][n_list + prefix] = __float_as_uint(hr.w);
      }
      n_list += (uint32_t)__popcll(mask);
      __builtin_amdgcn_wave_barrier();
      if (n_list >= 64u) {
         shade(list[0][lane], list[1][lane], entry(lane), true);
         n_hits += 64u;
         const uint32_t rest = n_list - 64u;  // move the tail (at most 63 entries) to the front: one wave, LDS operations execute in order
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
      shade(lane < n_list ? list[0][lane] : 0u, lane < n_list ? list[1][lane] : 0u, lane < n_list ? entry(lane) : make_float4(0.0f, 0.0f, 0.0f, 0.0f), lane < n_list);
      n_hits += n_list;
   }
   if (n_missed) flush_misses(n_missed);
   // closest_hits: per-block sum, one atomic per block (n_hits is wave-uniform)
   if (lane_id() == 0 && n_hits) atomicAdd(&s_hits, n_hits);
   __syncthreads();
   if (threadIdx.x == 0 && s_hits) atomicAdd(&stats->closest_hits, (unsigned long long)s_hits);
}

// ------------------------------------------------------------------------------------------
// primary_shade - bounce 0 of a pass whose primary rays need nothing stored (SamplePlan::fused_primary: camera grid, primary_implicit,
// slim state, no pixel handed to the tree): k_generate, k_trace_camera_grid and k_shade_hit(0) in one kernel. A lane stands at its
// path's pixel: the primary ray from the id (primary_state), the pixel's list (camera_list_walk: k_trace_camera_grid's walk), then a miss
// goes to bounce 0's Q_MISS as (0, id) - k_shade_miss needs the id alone there - and a hit is shaded where it was found
// (shade_hit_path: k_shade_hit's body). No id queue, no hit plane, no count of bounce 0's RAY queue: those only carried values from one
// of the three kernels to the next. One wave per run of 64 consecutive path ids, as k_generate: the run's shard (shard_of_run) is
// wave-uniform and every append of the wave goes to that shard's counters and segments. 97 % of the primary rays of the benchmark's
// scenes hit, so the hits are shaded as they lie - no compaction across runs.
// ------------------------------------------------------------------------------------------
template <bool SLIM>
__global__ __launch_bounds__(kBlock, kShadeHitBlocks) void k_primary_shade(FrameParams fp, SceneDev sc, PathState ps, Control* ctl, DeviceStats* stats, SunGridDev g) {
   static_assert(SLIM, "the plan asks for this kernel under the slim state alone");
   __shared__ float s_lut[256];
   s_lut[threadIdx.x] = sc.unorm_lut[threadIdx.x];
   __shared__ MeshShade s_mesh[kLdsMeshes];
   __shared__ TexInfo s_tex[kLdsTextures];
   const uint32_t n_lds_mesh = sc.num_meshes < kLdsMeshes ? sc.num_meshes : kLdsMeshes;
   const uint32_t n_lds_tex = sc.num_textures < kLdsTextures ? sc.num_textures : kLdsTextures;
   __shared__ uint32_t s_hits;
   if (threadIdx.x == 0) s_hits = 0;
   if (threadIdx.x < n_lds_mesh) s_mesh[threadIdx.x] = sc.meshes[threadIdx.x];
   if (threadIdx.x < n_lds_tex) s_tex[threadIdx.x] = sc.textures[threadIdx.x];
   __syncthreads();
   const uint32_t n = fp.n_owned * fp.batch_frames;  // owned pixels x frames of the batch
   const uint32_t lane = lane_id();
   const uint32_t runs = (n + 63) / 64;
   const float4* __restrict__ tris = sc.tris;
   uint32_t n_hits = 0, n_tris = 0;  // n_hits: wave-uniform
   for (uint32_t run = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); run < runs; run += gridDim.x * kWavesPerBlock) {
      const uint32_t shard = __builtin_amdgcn_readfirstlane(shard_of_run(run));
      const uint32_t seg = shard * ps.shard_cap;
      const uint32_t id = run * 64u + lane;
      const bool own = id < n;
      float4 ro = make_float4(0, 0, 0, 0), rd = make_float4(0, 0, 0, 0);
      float4 hr = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kEmptyRef));
      if (own) {
         primary_state(fp, id, ro, rd);
         const uint32_t k = id % fp.n_owned;
         const uint32_t pix = fp.owned_pixels ? fp.owned_pixels[k] : k;
         const uint32_t px = pix % fp.W, py = pix / fp.W;
         const uint32_t cell = (py + 1) * g.nx + (px + 1);
         const uint32_t e = g.cell_start[cell], end = g.cell_start[cell + 1];
         // (a list beyond max_walk is not sorted: walked whole. The plan sees to it that none is longer than k_trace_camera_grid would walk.)
         const Hit best = camera_list_walk<false>(g, tris, e, end, end - e <= g.max_walk, v3(ro.x, ro.y, ro.z), v3(rd.x, rd.y, rd.z), n_tris);
         hr = make_float4(best.t, best.u, best.v, __uint_as_float(best.idx));
      }
      const bool is_hit = __float_as_uint(hr.w) != kEmptyRef;
      const bool is_miss = own && !is_hit;
      if (__ballot(is_miss) != 0ull) {  // wave-uniform: every lane of the wave takes part in the append
         const uint32_t slot = wave_append(&ctl->q_count[qc_index(0, Q_MISS, shard)], is_miss);
         if (is_miss) st_stream(reinterpret_cast<uint2*>(ps.queue[4]) + seg + slot, make_uint2(0u, id));
      }
      const unsigned long long mask = __ballot(is_hit);
      if (mask == 0ull) continue;
      const HitShadeCtx hx{s_lut, s_mesh, s_tex, n_lds_mesh, n_lds_tex, seg, ps.set[0], ps.set[1], ps.queue[1] + seg, &ctl->q_count[qc_index(1, Q_RAY, shard)],
                           ps.queue[2] + seg, &ctl->q_count[qc_index(0, Q_LIGHT, shard)]};
      shade_hit_path<SLIM, true>(fp, sc, ps, hx, 0u, id, 0u, hr, is_hit, ro, rd);
      n_hits += (uint32_t)__popcll(mask);
   }
   if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&stats->rays[UH_RAY_PRIMARY], (unsigned long long)n);
   // closest_hits: per-block sum, one atomic per block
   if (lane == 0 && n_hits) atomicAdd(&s_hits, n_hits);
   __syncthreads();
   if (threadIdx.x == 0 && s_hits) atomicAdd(&stats->closest_hits, (unsigned long long)s_hits);
}

// The paths still alive after the last bounce (the ray queue shade_hit(num_bounces - 1) built): their radiance - with what the
// last bounce's shadow rays added - and their raygen RNG word go to the per-id array k_finish_sample and the next sample's
// k_generate read (rgen:127, :28-31). Dense reads by queue position, one 16-byte store per surviving path. With sun verdicts the
// last bounce's sun term is added here: one word per wave, and the throughput of the lit survivors.
// (Not launched for a pass with the slim state: the FINAL sun kernels of its last bounce store these records themselves.)
__global__ __launch_bounds__(kBlock) void k_flush_survivors(FrameParams fp, PathState ps, Control* ctl) {
   const ShardCtx sx = shard_ctx();
   const uint32_t seg = sx.shard * ps.shard_cap, b = fp.num_bounces;
   const uint32_t count = ctl->q_count[qc_index(b, Q_RAY, sx.shard)];
   const uint32_t* __restrict__ queue = ps.queue[b & 1] + seg;
   const PathRecs rec = ps.set[b & 1];
   for (uint32_t i = sx.lb * kBlock + threadIdx.x; i < count; i += sx.nb * kBlock) {
      const uint32_t id = ld_stream(queue + i);
      float4 rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (rad_stored(fp, b)) rad = ld_rec(rec_quad(rec, seg + i, REC_RAD));
      const float4 ro = ld_rec(rec_quad(rec, seg + i, REC_ORIGIN));
      if (fp.sun_verdicts) {
         const uint32_t i0 = __builtin_amdgcn_readfirstlane(i - lane_id());  // (the first active lane's: lanes hold consecutive positions)
         if ((*sun_lit_word(ps, seg + i0) >> lane_id()) & 1ull) rad = shadow_lit<false>(ld_rec(rec_quad(rec, seg + i, REC_THR)), rad);
      }
      st_stream(ps.radf + id, make_float4(rad.x, rad.y, rad.z, ro.w));
   }
}

// ------------------------------------------------------------------------------------------
// finish_sample — reference.rgen:127 (pixelColor += radiance) and, after the last sample of the
// frame, rgen:130-144 (accumulate, sRGB, store both images)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_finish_sample(FrameParams fp, PathState ps, Images im, uint32_t sample, bool last) {
   for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < fp.n_owned; k += gridDim.x * kBlock) {
      const uint32_t pix = fp.owned_pixels ? fp.owned_pixels[k] : k;
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      bool acc_loaded = false;
      uint32_t total = fp.total_samples;
      // frames of the batch in order: each applies the reference's accumulate tail with ITS total_samples
      for (uint32_t f = 0; f < fp.batch_frames; f++) {
         const uint32_t id = f * fp.n_owned + k;
         float4 pc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         if (sample != 0) pc = ps.pixcol[id];
         if (fp.num_bounces != 0) rad = ps.radf[id];  // where the path ended (miss, absorption, or the flush after the last bounce); with zero bounces no kernel ever wrote one
         pc = make_float4(pc.x + rad.x, pc.y + rad.y, pc.z + rad.z, 0.0f);                  // rgen:127
         if (!last) {
            ps.pixcol[id] = pc;
            continue;
         }
         total = fp.total_samples_of[f];
         if (total != fp.samples_per_frame) {                                               // rgen:131-134
            if (!acc_loaded) acc = im.accumulation[pix];
         } else {
            acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         }
         acc_loaded = true;
         if (total <= fp.accumulation_limit) acc = make_float4(acc.x + pc.x, acc.y + pc.y, acc.z + pc.z, 0.0f);  // rgen:136-138
         acc.w = 0.0f;
      }
      if (!last) continue;
      im.accumulation[pix] = acc;                                                            // rgen:143
      im.output[pix] = resolve_color(acc, total, fp.accumulation_limit);                     // rgen:144
   }
}

__global__ __launch_bounds__(kBlock) void k_resolve(Images im, uint32_t n, uint32_t total_samples, uint32_t limit) {
   for (uint32_t id = blockIdx.x * kBlock + threadIdx.x; id < n; id += gridDim.x * kBlock)
      im.output[id] = resolve_color(im.accumulation[id], total_samples, limit);
}

// ------------------------------------------------------------------------------------------
// G-buffer position by primary-ray cast (replaces the raster gbuffer_pass for this input only:
// utopian/src/renderers/gbuffer.rs:11-52, shaders/gbuffer/gbuffer.frag:47; clear colour
// (1,1,1,0): utopian/src/pass.rs:210-214)
// ------------------------------------------------------------------------------------------
// ray j of the cast is the primary ray of pixel spans.pixel_of(j): the rays of a rank's rows lie densely in the ray arrays
__global__ __launch_bounds__(kBlock) void k_gbuffer_generate(FrameParams fp, RawRays ps, RowSpans spans) {
   const uint32_t n = spans.total();
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
      const uint32_t id = spans.pixel_of(j);
      V3 o, d;
      primary_ray(fp, id % fp.W, id / fp.W, 0.5f, 0.5f, o, d);
      ps.ray_o[j] = make_float4(o.x, o.y, o.z, 0.001f);
      ps.ray_d[j] = make_float4(d.x, d.y, d.z, 10000.0f);
   }
}
__global__ __launch_bounds__(kBlock) void k_gbuffer_resolve(FrameParams fp, RawRays ps, Images im, DeviceStats* stats, RowSpans spans, uint32_t counted) {
   const uint32_t n = spans.total();
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
      const uint32_t id = spans.pixel_of(j);
      float4 h = ps.hit[j];
      if (__float_as_uint(h.w) != kEmptyRef) {
         float4 ro = ps.ray_o[j], rd = ps.ray_d[j];
         V3 p = v3(ro.x, ro.y, ro.z) + h.x * v3(rd.x, rd.y, rd.z);
         im.gbuffer_pos[id] = make_float4(p.x, p.y, p.z, 1.0f);
      } else {
         im.gbuffer_pos[id] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      }
   }
   if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&stats->rays[UH_RAY_GBUFFER], (unsigned long long)counted);
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
uint32_t query_trace_occupancy() {
   int a = 0, b = 0;
   if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_trace_closest<false>, kBlock, 0) != hipSuccess) a = 4;
   if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_trace_shadow<false, false>, kBlock, 0) != hipSuccess) b = 4;
   int m = a < b ? a : b;
   if (m < 1) m = 1;
   if (m > 8) m = 8;
   return (uint32_t)m;
}

void launch_generate(const LaunchCfg& c, const FrameParams& fp, const PathState& ps, Control* ctl, uint32_t sample) {
   k_generate<<<stream_grid(c, fp.n_owned * fp.batch_frames), kBlock, 0, c.stream>>>(fp, ps, ctl, sample);
}

// closest-hit traversal over a sharded queue of path ids (sharded) or over n raw rays
static void launch_closest(const LaunchCfg& c, dim3 grid, const SceneDev& sc, bool sharded, const float4* ray_o, const float4* ray_d, float4* hit,
                           uint32_t shard_cap, Control* ctl, DeviceStats* stats, uint32_t bounce, uint32_t cursor_slot, int ray_kind, uint32_t n,
                           const uint32_t* listed = nullptr) {
   if (c.count_visits && sharded)
      k_trace_closest<true><<<grid, kBlock, 0, c.stream>>>(sc, sharded, ray_o, ray_d, hit, shard_cap, ctl, stats, bounce, cursor_slot, ray_kind, n, listed);
   else
      k_trace_closest<false><<<grid, kBlock, 0, c.stream>>>(sc, sharded, ray_o, ray_d, hit, shard_cap, ctl, stats, bounce, cursor_slot, ray_kind, n, listed);
}

void launch_trace_closest(const LaunchCfg& c, const SceneDev& sc, const PathState& ps, Control* ctl, DeviceStats* stats, uint32_t bounce,
                          uint32_t cursor_slot, int ray_kind) {
   const PathRecs& rec = ps.set[bounce & 1];
   launch_closest(c, closest_grid(c), sc, true, rec_quad(rec, 0, REC_ORIGIN), rec_quad(rec, 0, REC_DIR), ps.hit, ps.shard_cap, ctl, stats, bounce, cursor_slot, ray_kind, 0);
}

// bounce 0 of the path tracer through the camera grid, then the tree walk for the rays of the pixels with long lists
void launch_trace_camera_grid(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const PathState& ps, Control* ctl, DeviceStats* stats, uint32_t cursor_slot_grid,
                              uint32_t cursor_slot_tree, const SunGridDev& g, bool leftovers_possible) {
   const dim3 grid = sharded_grid(c.num_cus * 8);
   if (c.count_visits)
      k_trace_camera_grid<true><<<grid, kBlock, 0, c.stream>>>(sc, fp, ps, ctl, stats, cursor_slot_grid, g);
   else
      k_trace_camera_grid<false><<<grid, kBlock, 0, c.stream>>>(sc, fp, ps, ctl, stats, cursor_slot_grid, g);
   if (!leftovers_possible) return;  // no pixel lists more than the grid kernel walks itself
   const PathRecs& rec = ps.set[0];
   launch_closest(c, closest_grid(c), sc, true, rec_quad(rec, 0, REC_ORIGIN), rec_quad(rec, 0, REC_DIR), ps.hit, ps.shard_cap, ctl, stats, 0, cursor_slot_tree, UH_RAY_PRIMARY, 0, ps.queue[3]);
}

void launch_shade_miss(const LaunchCfg& c, const FrameParams& fp, const PathState& ps, Control* ctl, DeviceStats* stats, uint32_t bounce) {
   // the bounce's misses are a dense queue (Q_MISS, written by k_shade_hit): every lane shades one; the count is on the
   // device, so the grid is sized for the paths the wavefront started with
   const dim3 full = shade_grid(c, fp.n_owned * fp.batch_frames), lean = sharded_grid(c.num_cus * 8);  // blocks per CU 2 / 4 / 6 / 8: 7,599 / 7,613-7,656 / 7,699 / 7,676-7,678 Mrays/s (round 4)
   as_constant(fp.slim_state != 0, [&](auto slim) { k_shade_miss<decltype(slim)::value><<<full.x < lean.x ? full : lean, kBlock, 0, c.stream>>>(fp, ps, ctl, stats, bounce); });
}

void launch_shade_hit(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const PathState& ps, const Images& im, Control* ctl,
                      DeviceStats* stats, uint32_t bounce) {
   as_constant(fp.slim_state != 0, [&](auto slim) { k_shade_hit<decltype(slim)::value><<<shade_grid(c, fp.W * fp.H), kBlock, 0, c.stream>>>(fp, sc, ps, ctl, stats, bounce); });
}
// bounce 0 of a pass with SamplePlan::fused_primary, in place of launch_generate, launch_trace_camera_grid and launch_shade_hit(0)
void launch_primary_shade(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const PathState& ps, Control* ctl, DeviceStats* stats, const SunGridDev& g) {
   k_primary_shade<true><<<stream_grid(c, fp.n_owned * fp.batch_frames), kBlock, 0, c.stream>>>(fp, sc, ps, ctl, stats, g);
}
// the sun rays of this bounce are the last of a pass with the slim state: they store the surviving paths' radiance themselves
static bool final_sun_rays(const FrameParams& fp, uint32_t bounce) { return fp.slim_state != 0 && bounce + 1 == fp.num_bounces; }

void launch_flush_survivors(const LaunchCfg& c, const FrameParams& fp, const PathState& ps, Control* ctl) {
   k_flush_survivors<<<shade_grid(c, fp.n_owned * fp.batch_frames), kBlock, 0, c.stream>>>(fp, ps, ctl);
}

void launch_trace_shadow(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const PathState& ps, Control* ctl, DeviceStats* stats,
                         uint32_t bounce, uint32_t cursor_slot, bool light, bool sun_leftovers) {
   // sun_leftovers: what the sun grid handed to the tree (queue 3); behind a grid kernel that left verdicts they set their bits
   as_constant(c.count_visits, [&](auto count) {
      auto go = [&](auto is_light, auto verdict, auto final) {
         k_trace_shadow<decltype(count)::value, decltype(is_light)::value, decltype(verdict)::value, decltype(final)::value><<<shadow_grid(c), kBlock, 0, c.stream>>>(
            sc, fp, ps, ctl, stats, bounce, cursor_slot, sun_leftovers);
      };
      if (light) go(std::true_type{}, std::false_type{}, std::false_type{});
      else if (sun_leftovers && final_sun_rays(fp, bounce)) go(std::false_type{}, std::true_type{}, std::true_type{});
      else if (sun_leftovers && fp.sun_verdicts) go(std::false_type{}, std::true_type{}, std::false_type{});
      else go(std::false_type{}, std::false_type{}, std::false_type{});
   });
}

void launch_trace_sun_grid(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const PathState& ps, Control* ctl, DeviceStats* stats, uint32_t bounce,
                           uint32_t cursor_slot, const SunGridDev& g) {
   const dim3 grid = sharded_grid(c.num_cus * 8);
   as_constant(c.count_visits, [&](auto count) {
      as_constant(g.recs != nullptr, [&](auto inl) {
         auto go = [&](auto verdict, auto final) {
            k_trace_sun_grid<decltype(count)::value, decltype(inl)::value, decltype(verdict)::value, decltype(final)::value><<<grid, kBlock, 0, c.stream>>>(
               sc, fp, ps, ctl, stats, bounce, cursor_slot, g);
         };
         if (final_sun_rays(fp, bounce)) go(std::true_type{}, std::true_type{});
         else if (fp.sun_verdicts != 0) go(std::true_type{}, std::false_type{});
         else go(std::false_type{}, std::false_type{});
      });
   });
}

void launch_finish_sample(const LaunchCfg& c, const FrameParams& fp, const PathState& ps, const Images& im, uint32_t sample, bool last) {
   k_finish_sample<<<stream_grid(c, fp.n_owned), kBlock, 0, c.stream>>>(fp, ps, im, sample, last);
}

void launch_resolve(const LaunchCfg& c, const Images& im, uint32_t W, uint32_t H, uint32_t total_samples, uint32_t limit) {
   k_resolve<<<stream_grid(c, W * H), kBlock, 0, c.stream>>>(im, W * H, total_samples, limit);
}

// the cast of launch_gbuffer and of the hybrid graph's G-buffer (kernel_common.h)
void launch_gbuffer_cast(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const RawRays& rr, const RowSpans& spans, DeviceStats* stats,
                         const SunGridDev* camera_grid) {
   const uint32_t n = spans.total();
   k_gbuffer_generate<<<stream_grid(c, n), kBlock, 0, c.stream>>>(fp, rr, spans);
   if (camera_grid)
      k_gbuffer_camera_grid<<<stream_grid(c, n), kBlock, 0, c.stream>>>(sc, rr, spans, fp.W, *camera_grid);
   else {
      const uint32_t full = c.num_cus * c.closest_blocks_per_cu, need = (n + kBlock - 1) / kBlock;
      launch_closest(c, dim3(need < full ? need : full), sc, false, rr.ray_o, rr.ray_d, rr.hit, 0, nullptr, stats, 0, 0, 0, n);
   }
}

void launch_gbuffer(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const RawRays& ps, const Images& im, DeviceStats* stats, const RowSpans& spans, uint32_t counted,
                    const SunGridDev* camera_grid) {
   const uint32_t n = spans.total();
   if (n == 0) return;
   launch_gbuffer_cast(c, fp, sc, ps, spans, stats, camera_grid);
   k_gbuffer_resolve<<<stream_grid(c, n), kBlock, 0, c.stream>>>(fp, ps, im, stats, spans, counted);
}

void launch_trace_closest_raw(const LaunchCfg& c, const SceneDev& sc, const float4* ray_o, const float4* ray_d, float4* hit, uint32_t n) {
   // a grid that fills the chip once; smaller queries get one block per 256 rays
   const uint32_t full = c.num_cus * c.closest_blocks_per_cu, need = (n + kBlock - 1) / kBlock;
   launch_closest(c, dim3(need < full ? (need ? need : 1) : full), sc, false, ray_o, ray_d, hit, 0, nullptr, nullptr, 0, 0, 0, n);
}
void launch_trace_any_raw(const LaunchCfg& c, const SceneDev& sc, const float4* ray_o, const float4* ray_d, uint32_t* occluded, uint32_t n) {
   k_trace_any_raw<<<stream_grid(c, n), kBlock, 0, c.stream>>>(sc, ray_o, ray_d, occluded, n);
}

}  // namespace uh
