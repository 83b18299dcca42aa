// traversal.h — the BVH4 walk every ray-tracing kernel shares (kernels.hip, path_fused.hip, hybrid_kernels.hip): the triangle and node
// tests, the per-lane traversal state and its LDS stack, the batch walk, and the persistent waves' ray refill from an LDS pool.
// The comments are the record of what was measured.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"
#include "node_slab.h"

namespace uh {

constexpr int kSunRaysPerLane = 2;   // k_trace_sun_grid (inline records): chains of dependent loads a lane keeps in flight
constexpr int kShadeHitBlocks = 4;   // blocks per CU the register budget of k_shade_hit is sized for
constexpr int kLdsStack = 16;        // per-lane traversal stack entries kept in LDS (16 KiB per 256-thread block)
constexpr int kSpillStack = (int)kTraversalStackEntries - kLdsStack;             // overflow entries in private memory (rarely touched); the host refuses trees deeper than the two together hold

// ------------------------------------------------------------------------------------------
// BVH4 traversal (thread per ray). Closest hit: min t over all triangles with tmin < t < tmax,
// ties broken by the smaller key (mesh << 22 | prim) — independent of traversal order, because
// the node test culls no triangle the triangle test accepts (node_slab.h: the builders' padded boxes, grown by the
// rounding of both tests at the ray's distance). Any hit: first triangle with tmin < t < tmax and t <= tlimit.
// ------------------------------------------------------------------------------------------
struct Hit {
   float t, u, v;
   uint32_t idx;  // packet index, kEmptyRef = miss
   uint32_t key;
};

__device__ __forceinline__ float dot_fma(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 cross_fma(V3 a, V3 b) {
   return v3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}

// Moeller-Trumbore on a baked packet (a = v0.xyz e1.x, b = e1.yz e2.xy, c = e2.z key): DESIGN.md "Arithmetic contract"
template <bool ANY>
__device__ __forceinline__ bool tri_compute(float4 a, float4 b, float4 c, uint32_t i, V3 o, V3 d, float tmin, float tlimit, Hit& best) {
   V3 v0 = v3(a.x, a.y, a.z), e1 = v3(a.w, b.x, b.y), e2 = v3(b.z, b.w, c.x);
   uint32_t key = __float_as_uint(c.y);
   V3 p = cross_fma(d, e2);
   float det = dot_fma(e1, p);
   if (det == 0.0f) return false;
   float inv = 1.0f / det;
   V3 tv = o - v0;
   float u = dot_fma(tv, p) * inv;
   if (!(u >= 0.0f && u <= 1.0f)) return false;
   V3 q = cross_fma(tv, e1);
   float v = dot_fma(d, q) * inv;
   if (!(v >= 0.0f && u + v <= 1.0f)) return false;
   float t = dot_fma(e2, q) * inv;
   if (!(t > tmin)) return false;
   if (ANY) {
      return t < best.t && t <= tlimit;
   } else {
      if (t < best.t || (t == best.t && key < best.key)) {
         best.t = t;
         best.u = u;
         best.v = v;
         best.idx = i;
         best.key = key;
         return true;
      }
      return false;
   }
}
template <bool ANY>
__device__ __forceinline__ bool tri_test(const float4* __restrict__ tris, uint32_t i, V3 o, V3 d, float tmin, float tlimit, Hit& best) {
   float4 a = tris[kTriStride16 * (size_t)i + 0], b = tris[kTriStride16 * (size_t)i + 1], c = tris[kTriStride16 * (size_t)i + 2];
   return tri_compute<ANY>(a, b, c, i, o, d, tmin, tlimit, best);
}

__device__ __forceinline__ float safe_rcp_dir(float x) {
   // the slab test only has to be conservative, and its margin (node_slab.h: 2^-16 of the node's reach, measured with idir an ulp
   // off either way) is 256 times the 1-ulp error of the hardware reciprocal: no IEEE division here; a zero component becomes
   // +-1e-30 so no inf/NaN appears
   return __builtin_amdgcn_rcpf(fabsf(x) < 1e-30f ? copysignf(1e-30f, x) : x);
}

struct Trav {
   V3 o, d, idir;
   float tmin, tlimit;
   Hit best;
   int sp;
   uint32_t cur;
};

__device__ __forceinline__ void trav_init(Trav& t, float4 ro, float4 rd, float tmin, float tmax, float tlimit) {
   t.o = v3(ro.x, ro.y, ro.z);
   t.d = v3(rd.x, rd.y, rd.z);
   t.idir = v3(safe_rcp_dir(t.d.x), safe_rcp_dir(t.d.y), safe_rcp_dir(t.d.z));
   t.tmin = tmin;
   t.tlimit = tlimit;
   t.best.t = tmax;
   t.best.u = t.best.v = 0.0f;
   t.best.idx = kEmptyRef;
   t.best.key = 0xffffffffu;
   t.sp = 0;
   t.cur = 0;
}

__device__ __forceinline__ void trav_push(Trav& t, uint32_t* lds_col, uint32_t* spill, uint32_t ref) {
   if (t.sp < kLdsStack)
      lds_col[t.sp * 64] = ref;
   else if (t.sp < kLdsStack + kSpillStack)
      spill[t.sp - kLdsStack] = ref;
   else
      return;
   t.sp++;
}
__device__ __forceinline__ uint32_t trav_pop(Trav& t, const uint32_t* lds_col, const uint32_t* spill) {
   if (t.sp == 0) return kEmptyRef;
   t.sp--;
   if (t.sp < kLdsStack) {
      // inline asm: written as `sp < kLdsStack ? lds_col[..] : spill[..]` hipcc selects between the LDS and the scratch
      // pointer and issues ONE flat_load - every pop then takes a slot of the vector memory addresser, the unit the
      // traversal kernels load most (one slot per lane and load, profiles/r02_microbench_rates.txt)
      uint32_t v;
      const uint32_t at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint32_t*)lds_col + 256u * (uint32_t)t.sp;
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(at) : "memory");
      return v;
   }
   return spill[t.sp - kLdsStack];
}

// one interior node (Node4C, 48 B = three loads): slab-test the 4 children, continue with the nearest, push
// the other hits. plane = origin + scale * q  =>  t = q * (scale * idir) + (origin - o) * idir -+ the margin of this ray at this node (node_slab.h).
//   w0 = origin.xyz, step exponents (the node's FRAME) ; w1 = qlo.xyz, qhi.x ; w2 = qhi.y, qhi.z, child_base | n_tri << 29, tri_base
// Child references are implicit (bvh.h): slot k is triangle packet tri_base + k below n_tri, node child_base + k - n_tri above.
// Instruction diet: the near / far plane words are picked once per axis by the sign of idir instead of min/max per
// plane; an empty slot is an inverted box, and since the margin can open it, slots are counted against n_child (a bit
// field of the frame word that is loaded anyway); only the nearest child is fully ordered
// (3 comparators); pushes are branch-free (write always, advance the stack pointer by the hit bit).
// Returns false when no child was hit: the caller pops (trav_step pops once for its node lanes and its leaf lanes together).
// CAP (closest-hit order, k_path_fused): children beyond t.tlimit are culled as in a visibility walk - the kernel's shadow rays go
// through the closest-hit walk (occluded <=> the closest hit lies within the limit) beside the other lanes' bounce rays
template <bool ANY, bool CAP = false>
__device__ __forceinline__ bool node_compute(const uint4 w0, const uint4 w1, const uint4 w2, Trav& t, uint32_t* lds_col, uint32_t* spill) {
   const uint32_t meta = w0.w;
   // a power-of-two step is its biased exponent moved to bits 23..30
   const float sx = __uint_as_float((meta & 0xffu) << 23), sy = __uint_as_float((meta << 15) & 0x7f800000u), sz = __uint_as_float((meta << 7) & 0x7f800000u);
   float ax, ay, az, bnx, bny, bnz, bfx, bfy, bfz;
   const float dx = __uint_as_float(w0.x) - t.o.x, dy = __uint_as_float(w0.y) - t.o.y, dz = __uint_as_float(w0.z) - t.o.z;
   const float growth = slab_node_growth(dx, sx, dy, sy, dz, sz);
   slab_axis(dx, sx, t.idir.x, growth, ax, bnx, bfx);
   slab_axis(dy, sy, t.idir.y, growth, ay, bny, bfy);
   slab_axis(dz, sz, t.idir.z, growth, az, bnz, bfz);
   const bool nx = t.idir.x < 0.0f, ny = t.idir.y < 0.0f, nz = t.idir.z < 0.0f;
   // qlo = (w1.x, w1.y, w1.z), qhi = (w1.w, w2.x, w2.y)
   const uint32_t qnx = nx ? w1.w : w1.x, qfx = nx ? w1.x : w1.w;
   const uint32_t qny = ny ? w2.x : w1.y, qfy = ny ? w1.y : w2.x;
   const uint32_t qnz = nz ? w2.y : w1.z, qfz = nz ? w1.z : w2.y;
   const float tcap = (ANY || CAP) ? fminf(t.best.t, t.tlimit) : t.best.t;  // closest: tlimit is +inf
   float tn[4];
   const uint32_t n_tri = w2.z >> kChildBaseBits, n_child = (meta >> kMetaChildShift) & 7u;
   const uint32_t tri0 = kLeafBit | w2.w, node0 = (w2.z & kChildBaseMask) - n_tri;
   uint32_t cr[4];
#pragma unroll
   for (int k = 0; k < 4; k++) cr[k] = ((uint32_t)k < n_tri ? tri0 : node0) + (uint32_t)k;
   bool hit[4];
#pragma unroll
   for (int k = 0; k < 4; k++) {
      const float t0x = slab_t((qnx >> (8 * k)) & 0xffu, ax, bnx), t1x = slab_t((qfx >> (8 * k)) & 0xffu, ax, bfx);
      const float t0y = slab_t((qny >> (8 * k)) & 0xffu, ay, bny), t1y = slab_t((qfy >> (8 * k)) & 0xffu, ay, bfy);
      const float t0z = slab_t((qnz >> (8 * k)) & 0xffu, az, bnz), t1z = slab_t((qfz >> (8 * k)) & 0xffu, az, bfz);
      const float tnear = fmaxf(fmaxf(t0x, t0y), fmaxf(t0z, t.tmin));
      const float tfar = fminf(fminf(t1x, t1y), fminf(t1z, tcap));
      hit[k] = tnear <= tfar && (uint32_t)k < n_child;  // the margin can open an empty slot's inverted box: count the slots
      tn[k] = hit[k] ? tnear : INFINITY;
   }
   if (ANY) {
      // visibility walk: no ordering network. The order of the children does not matter to an unoccluded ray (it visits
      // them all); an occluded one ends sooner if the likelier occluder comes first. The builders store a node's node
      // children in ascending surface area behind its triangle children (bvh_build.cpp, lbvh.hip), and the walk takes the
      // hit children from the HIGHEST slot down: biggest subtree first, triangles last (tools/any_order_ab.sh: 13.1 ->
      // 10.6 node visits per sun shadow ray). The other hits are pushed, lowest slot first, so that they pop in the same order.
      const bool any = hit[0] || hit[1] || hit[2] || hit[3];
      const uint32_t next = hit[3] ? cr[3] : hit[2] ? cr[2] : hit[1] ? cr[1] : cr[0];
      const bool p2 = hit[2] && hit[3], p1 = hit[1] && (hit[3] || hit[2]), p0 = hit[0] && (hit[3] || hit[2] || hit[1]);
      if (t.sp + 3 <= kLdsStack) {
         uint32_t* p = lds_col + t.sp * 64;
         p[0] = cr[0];
         p += (p0 ? 1 : 0) * 64;
         p[0] = cr[1];
         p += (p1 ? 1 : 0) * 64;
         p[0] = cr[2];
         t.sp += (p0 ? 1 : 0) + (p1 ? 1 : 0) + (p2 ? 1 : 0);
      } else {
         if (p0) trav_push(t, lds_col, spill, cr[0]);
         if (p1) trav_push(t, lds_col, spill, cr[1]);
         if (p2) trav_push(t, lds_col, spill, cr[2]);
      }
      t.cur = next;
      return any;
   }
   {
      // closest hit: bring the nearest hit to slot 0 (3 comparators); slots 1..3 stay unordered
      auto cswap = [&](int i, int j) {
         bool s = tn[j] < tn[i];
         float ta = s ? tn[j] : tn[i], tb = s ? tn[i] : tn[j];
         uint32_t ca = s ? cr[j] : cr[i], cb = s ? cr[i] : cr[j];
         tn[i] = ta;
         tn[j] = tb;
         cr[i] = ca;
         cr[j] = cb;
      };
      cswap(0, 1);
      cswap(2, 3);
      cswap(0, 2);
   }
   if (t.sp + 3 <= kLdsStack) {
      // branch-free pushes of slots 3, 2, 1
      uint32_t* p = lds_col + t.sp * 64;
      int h3 = tn[3] < INFINITY ? 1 : 0, h2 = tn[2] < INFINITY ? 1 : 0, h1 = tn[1] < INFINITY ? 1 : 0;
      p[0] = cr[3];
      p += h3 * 64;
      p[0] = cr[2];
      p += h2 * 64;
      p[0] = cr[1];
      t.sp += h3 + h2 + h1;
   } else {
      if (tn[3] < INFINITY) trav_push(t, lds_col, spill, cr[3]);
      if (tn[2] < INFINITY) trav_push(t, lds_col, spill, cr[2]);
      if (tn[1] < INFINITY) trav_push(t, lds_col, spill, cr[1]);
   }
   t.cur = cr[0];
   return tn[0] < INFINITY;
}

template <bool ANY>
__device__ __forceinline__ void node_step(const uint4* __restrict__ nodes, Trav& t, uint32_t* lds_col, uint32_t* spill) {
   const uint4* n = nodes + kNodeStride16 * (size_t)t.cur;
   const uint4 w0 = n[0], w1 = n[1], w2 = n[2];
   if (!node_compute<ANY>(w0, w1, w2, t, lds_col, spill)) t.cur = trav_pop(t, lds_col, spill);
}


// batch (if-if) traversal of one ray to its end: the batch kernels (variant 0) and the stand-alone any-hit query
template <bool ANY, bool COUNT>
__device__ __forceinline__ bool traverse(const SceneDev& sc, V3 o, V3 d, float tmin, float tmax, float tlimit, Hit& best, uint32_t* lds_col,
                                         uint32_t& n_nodes, uint32_t& n_tris) {
   Trav t;
   trav_init(t, make_float4(o.x, o.y, o.z, tmin), make_float4(d.x, d.y, d.z, tmax), tmin, tmax, ANY ? tlimit : INFINITY);
   uint32_t spill[kSpillStack];
   const uint4* __restrict__ nodes = sc.nodes;
   const float4* __restrict__ tris = sc.tris;
   bool occluded = false;
   // if-if: in a divergent wave both branches are issued every iteration, so a lane that the node step has just
   // sent to a triangle uses this iteration's triangle branch too instead of idling through it
   while (t.cur != kEmptyRef) {
      if (!(t.cur & kLeafBit)) {
         if (COUNT) n_nodes++;
         node_step<ANY>(nodes, t, lds_col, spill);
      }
      if (t.cur != kEmptyRef && (t.cur & kLeafBit)) {
         if (COUNT) n_tris++;
         if (tri_test<ANY>(tris, t.cur & ~kLeafBit, t.o, t.d, t.tmin, t.tlimit, t.best) && ANY) {
            occluded = true;
            break;
         }
         t.cur = trav_pop(t, lds_col, spill);
      }
   }
   best = t.best;
   return ANY ? occluded : (best.idx != kEmptyRef);
}

// persistent-thread batch fetch: lane 0 pulls the next 64-item batch of its shard
__device__ __forceinline__ uint32_t next_batch(uint32_t* cursor) {
   uint32_t base = 0;
   if (lane_id() == 0) base = atomicAdd(cursor, 64u);
   return __builtin_amdgcn_readfirstlane(base);
}

// blocks are bound to queue shards by blockIdx % kShards (device_types.h)
struct ShardCtx {
   uint32_t shard, lb, nb;  // shard id, this block's index within the shard, blocks per shard
};
__device__ __forceinline__ ShardCtx shard_ctx() {
   ShardCtx c;
   c.shard = blockIdx.x % kShards;
   c.lb = blockIdx.x / kShards;
   c.nb = gridDim.x / kShards;
   return c;
}

// ------------------------------------------------------------------------------------------
// Ray replacement ("refill") from a per-wave LDS ray pool.
//
// Thread-per-ray traversal leaves a lane idle from the moment its ray ends until the slowest ray of
// the wave ends (bounce rays: mean 18 steps against a wave maximum of 43, profiles/README.md). Here a
// wave is persistent and every lane whose ray has ended takes the next ray out of a 64-entry pool in
// LDS - a couple of ds_read_b128, no global round trip on the wave's critical path. The pool is kept
// fed by a three-stage pipeline, one stage per "refill event" (= the pool ran empty):
//    stage 1  lane 0 reserves the next 64-ray chunk of the shard's queue (one returning atomic),
//    stage 2  the 64 path ids of the chunk reserved one event earlier are loaded,
//    stage 3  the rays of the ids loaded one event earlier go global -> LDS by LDS-DMA
//             (global_load_lds_dwordx4: per-lane source address, 64 x 16 B contiguous in LDS).
// Every stage consumes what was issued a whole pool (about 20 wave iterations) earlier, so its wait
// finds the data there. The traversal kernels write nothing but their per-path result: no queue is
// built here (the shading kernels classify hits and misses themselves), so the loop has no atomic
// whose value it needs at once.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kPool = 64;

template <int NA>
struct alignas(16) RayPool {
   float4 v[NA][kPool];  // one LDS-DMA instruction fills one of these arrays
   uint32_t id[kPool];
};

__device__ __forceinline__ void dma16(const float4* gsrc, float4* lds_dst) {
   // lds_dst is wave-uniform; lane l's 16 bytes land at lds_dst + l. aux = 2: the nt cache policy
   __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 2);
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Where a wave's rays come from: a (shard segment of a) queue of path ids, or the identity (ray i = record i)
// when `queue` is null; chunks are handed out by an atomic cursor, or - `cursor` null - statically
// (chunk k of wave w = (k * num_waves + w) * 64).
struct RaySource {
   const uint32_t* queue;
   uint32_t count;
   uint32_t* cursor;
   uint32_t wave_index, num_waves;  // static chunk assignment only
};

template <int NA>
struct Feeder {
   // wave-uniform state (ballot / readfirstlane derived: lives in SGPRs)
   uint32_t pos = 0, n = 0;     // pool entries [pos, n) are unread
   uint32_t load_n = 0;         // entries the LDS-DMA in flight delivers
   uint32_t q_n = 0;            // valid lanes of q_id
   uint32_t static_k = 0;
   uint32_t iterations = 0;
   uint32_t q_base = 0, load_base = 0, pool_base = 0;  // first queue position of the chunk in q_id / in flight / in the pool
   bool loading = false, have_base = false, drained = false;
   // per-lane pipeline registers
   uint32_t r_base = 0;         // lane 0: what the newest cursor atomic returned
   uint32_t q_id = 0;           // path id of lane l's ray in the chunk that enters the pool next

   __device__ __forceinline__ bool empty() const { return pos >= n && !loading && q_n == 0 && !have_base && drained; }

   // the DMA issued one event ago has landed (its wait also covers every older load of the wave)
   __device__ __forceinline__ void land() {
      if (loading) {
         wait_vm0();
         pos = 0;
         n = load_n;
         pool_base = load_base;
         loading = false;
      }
   }

   // one refill event: called when the pool is empty and nothing is in flight
   template <typename SrcFn>
   __device__ __forceinline__ void advance(const RaySource& src, RayPool<NA>& pool, SrcFn&& source_of) {
      const uint32_t lane = lane_id();
      if (q_n) {  // stage 3
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the pool's last entries have been read
         if (lane < q_n) {
#pragma unroll
            for (int a = 0; a < NA; a++) dma16(source_of(a, q_id), pool.v[a]);
            pool.id[lane] = q_id;
         }
         load_n = q_n;
         load_base = q_base;
         loading = true;
         q_n = 0;
      }
      if (have_base) {  // stage 2
         const uint32_t b = __builtin_amdgcn_readfirstlane(r_base);
         have_base = false;
         if (b < src.count) {
            q_base = b;
            q_n = src.count - b < kPool ? src.count - b : kPool;
            if (lane < q_n) q_id = src.queue ? ld_stream(src.queue + b + lane) : b + lane;
         } else {
            drained = true;
         }
      }
      if (!drained) {  // stage 1
         if (src.cursor) {
            if (lane == 0) r_base = atomicAdd(src.cursor, kPool);
         } else {
            r_base = (static_k * src.num_waves + src.wave_index) * kPool;
            static_k++;
         }
         have_base = true;
      }
   }
};

// what a traversal wave does per iteration for its idle lanes; returns false when the wave is out of work.
// kRefill: idle lanes that make a refill worth its instructions (every lane that ends costs a pool read + trav_init);
// 4 / 8 / 16 measured 3.10 / 3.10 / 3.15 ms per frame (profiles/README.md)
constexpr int kRefill = 8;
template <int NA, typename SrcFn, typename TakeFn>
__device__ __forceinline__ bool refill_lanes(Feeder<NA>& f, const RaySource& src, RayPool<NA>& pool, bool lane_idle, SrcFn&& source_of, TakeFn&& take) {
   // exit condition every wave reaches whatever the data: a traversal step visits a node or a triangle once, so a
   // wave that has run this many iterations is not walking a tree any more (corrupt references) - leave
   if (++f.iterations > (1u << 24)) return false;
   const unsigned long long idle = __ballot(lane_idle);
   if (idle == 0ull) return true;
   const uint32_t n_idle = (uint32_t)__popcll(idle);
   f.land();
   const uint32_t avail = f.n - f.pos;
   if (avail != 0 && (n_idle >= (uint32_t)kRefill || n_idle == 64u)) {
      const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
      if (lane_idle && prefix < avail) take(f.pos + prefix);
      f.pos += n_idle < avail ? n_idle : avail;
   }
   if (f.pos >= f.n && !f.loading) {
      if (f.empty()) return n_idle != 64u || avail != 0;  // nothing left to hand out: done once every lane is idle
      f.advance(src, pool, source_of);
   }
   return true;
}

// one step of a lane's traversal; returns true when the ray has ended. ONE load phase per iteration: a lane at a node loads
// its node, a lane at a leaf its triangle, then both groups compute. A lane that reaches a leaf tests it an iteration later,
// but the wave waits for memory once per iteration (a chained node -> triangle step, two dependent round trips per
// iteration, measured 3.21 against 3.10 ms per frame: profiles/README.md).
template <bool ANY, bool COUNT, bool CAP = false>
__device__ __forceinline__ bool trav_step(const uint4* __restrict__ nodes, const float4* __restrict__ tris, Trav& t, uint32_t* lds_col, uint32_t* spill, bool& occluded,
                                          uint32_t& n_nodes, uint32_t& n_tris) {
   const bool at_node = !(t.cur & kLeafBit);
   const uint32_t packet = t.cur & ~kLeafBit;
   // nodes and triangle packets are both three-quad records: ONE address and ONE set of loads for the whole wave.
   // (Written as two branches, each with its own loads, the compiler gave the second branch's address the first
   // branch's destination registers and made it wait for them: the two groups' loads ran one after the other.)
   const uint4* rec = at_node ? nodes + kNodeStride16 * (size_t)packet : (const uint4*)tris + kTriStride16 * (size_t)packet;
   uint4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
   // the packet's last two dwords are padding: without this the compiler loads them in the node branch only (a fourth load)
   asm volatile("" : "+v"(w2.z), "+v"(w2.w));
   bool pop;  // one pop for both groups: an LDS read and its wait once per iteration, not once per branch
   if (at_node) {
      if (COUNT) n_nodes++;
      pop = !node_compute<ANY, CAP>(w0, w1, w2, t, lds_col, spill);
   } else {
      if (COUNT) n_tris++;
      const float4 ta = make_float4(__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z), __uint_as_float(w0.w));
      const float4 tb = make_float4(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z), __uint_as_float(w1.w));
      const float4 tc = make_float4(__uint_as_float(w2.x), __uint_as_float(w2.y), __uint_as_float(w2.z), __uint_as_float(w2.w));
      pop = true;
      if (tri_compute<ANY>(ta, tb, tc, packet, t.o, t.d, t.tmin, t.tlimit, t.best) && ANY) {
         occluded = true;
         t.cur = kEmptyRef;
         pop = false;
      }
   }
   if (pop) t.cur = trav_pop(t, lds_col, spill);
   return t.cur == kEmptyRef;
}

}  // namespace uh
