// item_walk.h — the persistent "item walk" the hybrid frame's ray passes share (k_hybrid_shadow, k_hybrid_restir_trace, k_rtao_trace,
// k_rtgi_trace, k_rtgi_shadow, k_glossy_trace, k_fog_trace): persistent waves with the LDS refill of traversal.h whose pool carries item numbers alone - items
// 0..count or queue[0..count), in static chunks - and the lane that takes an item makes its ray there. The kernels keep their loops:
//    __shared__ ItemWalkLds s_walk;
//    Trav t;
//    uint32_t spill[kSpillStack];
//    ItemWalk w(s_walk, t, spill, queue, count);
//    while (w.next(false, start)) { bool occluded; if (walk_step<kAny, kCount>(w, sc, occluded)) ...the lane's ray has ended... }
#pragma once
#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"
#include "traversal.h"

namespace uh {

// a block's LDS: the per-wave stack columns and item pools
struct ItemWalkLds {
   uint32_t stack[kWavesPerBlock][kLdsStack][64];
   RayPool<0> pool[kWavesPerBlock];
};

// A lane's walk state. The ray's Trav and spill[kSpillStack] are plain locals of the kernel, handed in: with the array as a member the
// whole struct goes to scratch, and with the Trav as a member the compiler allocates the walk's registers differently and the RTAO walk
// measured 1-2 % slower (profiles/hybrid_walk_resource_usage.txt).
struct ItemWalk {
   uint32_t* lds_col;
   uint32_t* spill;
   RayPool<0>* pool;
   RaySource src;
   Feeder<0> f;
   Trav& t;
   uint32_t n_nodes = 0, n_tris = 0;  // kCount walks: the lane's node visits and triangle tests

   __device__ __forceinline__ ItemWalk(ItemWalkLds& lds, Trav& t_, uint32_t* spill_, const uint32_t* queue, uint32_t count) : spill(spill_), t(t_) {
      const uint32_t wave = threadIdx.x >> 6;
      lds_col = &lds.stack[wave][0][lane_id()];
      pool = &lds.pool[wave];
      src.queue = queue;
      src.count = count;
      src.cursor = nullptr;
      src.wave_index = blockIdx.x * kWavesPerBlock + wave;
      src.num_waves = gridDim.x * kWavesPerBlock;
      t.cur = kEmptyRef;
      t.sp = 0;
   }

   __device__ __forceinline__ bool walking() const { return t.cur != kEmptyRef; }

   // One wave iteration's refill: a lane that neither walks nor waits takes the next item, and start(item) makes its ray (trav_init on
   // the kernel's t). False when the wave is out of work.
   template <typename Start>
   __device__ __forceinline__ bool next(bool waiting, Start&& start) {
      auto source_of = [](int, uint32_t) { return (const float4*)nullptr; };
      return refill_lanes<0>(f, src, *pool, !walking() && !waiting, source_of, [&](uint32_t slot) { start(pool->id[slot]); });
   }
};

// one step of a walking lane; true when its walk ended, occluded: an any-hit walk found a hit
template <bool kAny, bool kCount>
__device__ __forceinline__ bool walk_step(ItemWalk& w, const SceneDev& sc, bool& occluded) {
   occluded = false;
   return w.walking() && trav_step<kAny, kCount>(sc.nodes, sc.tris, w.t, w.lds_col, w.spill, occluded, w.n_nodes, w.n_tris);
}

}  // namespace uh
