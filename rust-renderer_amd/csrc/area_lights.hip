// area_lights.hip — emissive meshes as area lights of the hybrid frame (UH_HYBRID_AREA_LIGHTS; utopian_hip.h): the emitter table filled
// from the tree's own triangle packets (fill + maximum, integer weights, their prefix), which pixels cast and the emitters' own pixels,
// the samples (pick, point, geometry, the two shading halves) with their shadow rays queued, those rays through the any-hit walk, the
// per-pixel means in sample order, the tile filter and the composite into deferred_output; with their launchers.
// An extension: the reference leaves its diffuse light a "Todo". Arithmetic: DESIGN.md section 2 "Area lights";
// tests/area_light_reference.py restates it.
#include <hip/hip_runtime.h>

#include "bvh.h"
#include "device_math.h"
#include "device_scan.h"
#include "device_types.h"
#include "edge_filter.h"
#include "hybrid_shading.h"
#include "item_walk.h"
#include "kernel_common.h"
#include "traversal.h"

namespace uh {

static_assert(kBlock == 256, "k_area_sample and k_area_composite fill their 256-entry gamma table one entry per thread of the block");

// the bytes of a pixel's count word
constexpr uint32_t kAlLit = 1u, kAlOccluded = 1u << 8, kAlAway = 1u << 16;

// ---- the emitter table ------------------------------------------------------------------------------------------------------------------
// One lane per triangle packet of the tree, whatever its order: a packet of an emitter mesh writes its slot base[mesh] + prim - the
// packet's world-space v0, e1, e2, its key and its area 0.5 sqrt(dot(Ng, Ng)), Ng = cross(e1, e2) (not finite: 0) - and takes part in the
// maximum, an atomicMax on the bits of the non-negative floats: exact, whatever the order.
__global__ __launch_bounds__(kBlock) void k_area_fill(const float4* __restrict__ tris, uint32_t num_tris, AreaTableDev tab) {
   const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= num_tris) return;
   const float4* pk = tris + kTriStride16 * (size_t)i;
   const float4 a = pk[0], b = pk[1], c = pk[2];  // TriPacket: v0 | e1x ; e1y e1z e2x e2y ; e2z key pad pad
   const uint32_t key = __float_as_uint(c.y), mesh = key >> kPrimBits;
   if (mesh >= tab.num_meshes) return;
   const uint32_t base = tab.base[mesh];
   if (base == kNoEmitter) return;
   const uint32_t slot = base + (key & kPrimMask);
   if (slot >= tab.n) return;
   const V3 e1 = v3(a.w, b.x, b.y), e2 = v3(b.z, b.w, c.x);
   const V3 Ng = cross3(e1, e2);
   float area = 0.5f * sqrtf(dot3(Ng, Ng));
   if (!(area < INFINITY)) area = 0.0f;  // infinite or NaN
   tab.tri[3 * (size_t)slot] = make_float4(a.x, a.y, a.z, area);
   tab.tri[3 * (size_t)slot + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
   tab.tri[3 * (size_t)slot + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
   tab.keys[slot] = key;
   tab.areas[slot] = area;
   atomicMax(tab.amax, __float_as_uint(area));
}

// q of every slot: with amax = m 2^x (frexpf) and b = 31 - bit_length(n - 1), max(1, trunc(area 2^(b - x))) for an area > 0, else 0 -
// the largest is below 2^b, the sum at most n 2^b <= 2^31
__global__ __launch_bounds__(kBlock) void k_area_weights(AreaTableDev tab) {
   const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= tab.n) return;
   int x = 0;
   (void)frexpf(__uint_as_float(*tab.amax), &x);
   const int b = 31 - (32 - __clz((int)(tab.n - 1)));
   const float area = tab.areas[i];
   uint32_t q = 0;
   if (area > 0.0f) {
      q = (uint32_t)truncf(ldexpf(area, b - x));
      if (q < 1u) q = 1u;
   }
   tab.weights[i] = q;
   tab.cum[i] = q;  // (scanned in place behind this kernel)
   tab.tri[3 * (size_t)i + 1].w = __uint_as_float(q);
}

// cum: the exclusive scan plus the slot's own weight
__global__ __launch_bounds__(kBlock) void k_area_inclusive(AreaTableDev tab) {
   const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
   if (i < tab.n) tab.cum[i] += tab.weights[i];
}

// ---- the pass ---------------------------------------------------------------------------------------------------------------------------
// the material record of a pixel as deferred.frag:46-65 forms it
struct AreaSurface {
   float metallic, roughness, type;
   V3 bc;
};
__device__ __forceinline__ AreaSurface area_surface(const SceneDev& sc, float4 R4) {
   AreaSurface m{R4.x, R4.y, 0.0f, v3(1.0f, 1.0f, 1.0f)};
   const uint32_t material = (uint32_t)R4.w;                                                    // frag:46
   if (material < sc.num_meshes) {
      const MeshShade& ms = sc.meshes[material];
      m.metallic = R4.x * ms.metallic;                                                          // frag:52-58
      m.roughness = R4.y * ms.roughness;
      m.type = ms.type;
      m.bc = v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);
   }
   return m;
}

// Queue appends of this file, one atomic per BLOCK and kU items per thread: an atomic on one word costs some 12 ns whoever issues it, and
// one per wave of 64 items was the whole cost of the classify and of a sample pass (DESIGN.md section 4 "Area lights"). pred[u] says
// whether the thread's item u is appended, slot[u] receives its place: the waves' counts meet in LDS, thread 0 reserves the block's
// range, and a thread's place is the range's start + the waves before its own + the items of its wave before its own (ballots). Every
// thread of the block must call it, from uniform control flow. The queue's order is no output of the pass: every image is written by
// pixel and every record by sample number.
template <int kU>
__device__ __forceinline__ void block_append(uint32_t* counter, const bool (&pred)[kU], uint32_t (&slot)[kU], uint32_t (&s_wave)[kWavesPerBlock + 1]) {
   unsigned long long mask[kU];
   uint32_t n = 0;
   for (int u = 0; u < kU; u++) {
      mask[u] = __ballot(pred[u]);
      n += (uint32_t)__popcll(mask[u]);
   }
   const uint32_t wave = threadIdx.x >> 6;
   if (lane_id() == 0) s_wave[wave] = n;
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t sum = 0;
      for (int k = 0; k < kWavesPerBlock; k++) {
         const uint32_t c = s_wave[k];
         s_wave[k] = sum;
         sum += c;
      }
      s_wave[kWavesPerBlock] = sum ? atomicAdd(counter, sum) : 0u;
   }
   __syncthreads();
   uint32_t at = s_wave[kWavesPerBlock] + s_wave[wave];
   for (int u = 0; u < kU; u++) {
      slot[u] = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask[u], 0u));
      at += (uint32_t)__popcll(mask[u]);
   }
   __syncthreads();  // (the next call writes s_wave again)
}

// Every pixel's counts and images are zeroed; an emitter's pixel (position w != 0, material type 3) is counted and, with show_emitters,
// written (1, 1, 1) * intensity; the pixels that cast (RTAO's rule, no emitter, no mirror that holds its reflection, a table with
// weight in it) are queued, four pixels per thread and block_append.
constexpr int kAlClassifyItems = 4;
__global__ __launch_bounds__(kBlock) void k_area_classify(SceneDev sc, HybridDev hd, HybridFrameDev fd, AreaDev al) {
   __shared__ uint32_t s_wave[kWavesPerBlock + 1];
   const bool any = *al.tab.total != 0ull;
   const uint32_t n = hd.W * hd.H;
   uint32_t n_emit = 0;
   for (uint64_t base = (uint64_t)blockIdx.x * (kBlock * kAlClassifyItems); base < n; base += (uint64_t)gridDim.x * (kBlock * kAlClassifyItems)) {  // (block-uniform)
      bool queued[kAlClassifyItems];
      uint32_t pixel[kAlClassifyItems], slot[kAlClassifyItems];
      for (int u = 0; u < kAlClassifyItems; u++) {
         const uint64_t p = base + (uint64_t)u * kBlock + threadIdx.x;
         const uint32_t pix = pixel[u] = (uint32_t)p;
         queued[u] = false;
         if (p >= n) continue;
         al.counts[pix] = 0;
         al.diffuse[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         al.specular[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         if (hd.pos[pix].w == 0.0f) continue;
         const float type = area_surface(sc, hd.pbr[pix]).type;
         if (type == 3.0f) {
            n_emit++;
            if (al.show_emitters) {
               const float4 d = fd.deferred[pix];
               const float e = 1.0f * al.intensity;
               fd.deferred[pix] = make_float4(e, e, e, d.w);
            }
            continue;
         }
         V3 nn;
         queued[u] = any && rtao_normal(hd.nrm[pix], nn) && !(al.rt_on && type == 1.0f);
      }
      block_append<kAlClassifyItems>(al.counters, queued, slot, s_wave);
      for (int u = 0; u < kAlClassifyItems; u++)
         if (queued[u]) al.queue[slot[u]] = pixel[u];
   }
   wave_add(&al.counters[3], n_emit);
}

// the 32-bit output word of one step of the state: what random_float (device_math.h) converts
__device__ __forceinline__ uint32_t random_word(uint32_t& s) {
   s = s * 747796405u + 1u;
   uint32_t word = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
   return (word >> 22) ^ word;
}

// The samples, a streaming kernel: item i is sample (queue[i / samples], i % samples) - kOrder 0: a pixel's samples are neighbours in a
// wave - or (queue[i % pixels], i / pixels) - kOrder 1: a wave holds one sample of 64 consecutive queued pixels (measured: DESIGN.md
// section 4 "Area lights"). The lane picks its emitter (binary search of the inclusive prefix for the first slot above the target: integers
// only), its point, forms the geometry term and the two shading halves, stores them and appends its shadow ray (block_append, two items
// per thread: one atomic per 512 samples); an AWAY sample stores zeros and bumps its byte of the pixel's count word instead.
constexpr int kAlSampleItems = 2;
template <int kOrder>
__global__ __launch_bounds__(kBlock) void k_area_sample(SceneDev sc, HybridDev hd, AreaDev al) {
   __shared__ float s_gamma[256];  // pow(c / 255, 2.2) of every UNORM8 value: pow in double, rounded to float
   s_gamma[threadIdx.x] = (float)pow((double)((float)threadIdx.x / 255.0f), (double)2.2f);
   __syncthreads();
   const uint32_t pixels = al.counters[0], items = pixels * al.samples;
   const uint32_t total = (uint32_t)*al.tab.total;  // <= 2^31
   const float ftotal = (float)total;
   __shared__ uint32_t s_wave[kWavesPerBlock + 1];
   for (uint64_t first = (uint64_t)blockIdx.x * (kBlock * kAlSampleItems); first < items; first += (uint64_t)gridDim.x * (kBlock * kAlSampleItems)) {  // (block-uniform)
      bool casts[kAlSampleItems];
      uint32_t rays[kAlSampleItems], slots[kAlSampleItems];
      V3 origins[kAlSampleItems], points[kAlSampleItems];
      for (int u = 0; u < kAlSampleItems; u++) {
         const uint64_t item = first + (uint64_t)u * kBlock + threadIdx.x;
         bool cast = false;
         V3 o = v3(0.0f, 0.0f, 0.0f), Y = o;
         uint32_t ray = 0;
         if (item < items) {
            const uint32_t it = (uint32_t)item;
            uint32_t q, s;
            if (kOrder == 0) {
               q = it / al.samples;
               s = it % al.samples;
            } else {
               q = it % pixels;
               s = it / pixels;
            }
            const uint32_t pix = al.queue[q];
            ray = q * al.samples + s;
            uint32_t rng = init_rng(pix % hd.W, pix / hd.W, hd.W, (al.frame_base + s) ^ kAreaSeedXor);
            const uint32_t r = random_word(rng);
            float u1 = random_float(rng), u2 = random_float(rng);
            // the pick: the first slot whose inclusive prefix exceeds the target
            const uint32_t target = (uint32_t)(((uint64_t)r * total) >> 32);
            uint32_t lo = 0, hi = al.tab.n - 1;
            while (lo < hi) {
               const uint32_t mid = (lo + hi) >> 1;
               if (al.tab.cum[mid] > target)
                  hi = mid;
               else
                  lo = mid + 1;
            }
            const float4 t0 = al.tab.tri[3 * (size_t)lo], t1 = al.tab.tri[3 * (size_t)lo + 1], t2 = al.tab.tri[3 * (size_t)lo + 2];
            const V3 v0 = xyz(t0), e1 = xyz(t1), e2 = xyz(t2);
            const float area = t0.w, fq = (float)__float_as_uint(t1.w);
            if (u1 + u2 > 1.0f) {
               u1 = 1.0f - u1;
               u2 = 1.0f - u2;
            }
            Y = (v0 + u1 * e1) + u2 * e2;
            // the geometry term
            const float4 P4 = hd.pos[pix], N4 = hd.nrm[pix];
            const V3 P = xyz(P4), N = xyz(N4);
            const V3 Ng = cross3(e1, e2);
            const float ng2 = dot3(Ng, Ng);
            const V3 w = Y - P;
            const float d2 = dot3(w, w), dist = sqrtf(d2);
            const V3 l = v3(w.x / dist, w.y / dist, w.z / dist);
            const float cosL = fabsf(dot3(Ng, l)) / sqrtf(ng2);
            const float NdotL = dot3(N, l);
            const float invpdf = (area * ftotal) / fq;
            const float g0 = (cosL / d2) * invpdf;
            V3 ds = v3(0.0f, 0.0f, 0.0f), ss = ds;
            if (d2 > 0.0f && NdotL > 0.0f && cosL > 0.0f && g0 == g0) {
               const float G = fminf(g0, al.max_weight);
               const AreaSurface m = area_surface(sc, hd.pbr[pix]);
               const uchar4 A = hd.alb[pix];
               const V3 base = v3(s_gamma[A.x], s_gamma[A.y], s_gamma[A.z]) * m.bc;                // frag:61-65
               const V3 V = normalize3(v3(hd.eye[0], hd.eye[1], hd.eye[2]) - P);                    // lighting:26
               const LightHalves h = light_halves(surface_terms(N, V, base, m.metallic, m.roughness), N, V, l, NdotL, v3(G, G, G));
               ds = h.d, ss = h.s;
               V3 nn;
               rtao_normal(N4, nn);
               o = offset_ray(P, nn);
               cast = true;
            } else {
               atomicAdd(al.counts + pix, kAlAway);
            }
            al.rec_d[ray] = make_float4(ds.x, ds.y, ds.z, 0.0f);
            al.rec_s[ray] = make_float4(ss.x, ss.y, ss.z, 0.0f);
         }
         casts[u] = cast, rays[u] = ray, origins[u] = o, points[u] = Y;
      }
      block_append<kAlSampleItems>(al.counters + 1, casts, slots, s_wave);
      for (int u = 0; u < kAlSampleItems; u++)
         if (casts[u]) {
            al.rays[2 * (size_t)slots[u]] = make_float4(origins[u].x, origins[u].y, origins[u].z, __uint_as_float(rays[u]));
            al.rays[2 * (size_t)slots[u] + 1] = make_float4(points[u].x, points[u].y, points[u].z, 0.0f);
         }
   }
}

// One any-hit ray per queued record, an item walk (item_walk.h) over the record numbers: from o toward Y, tmin 0.001, tmax 0.999 |Y - o|.
// An occluded ray zeroes its sample's two records; every ray bumps its byte of the pixel's count word (a 32-bit atomic on the word: a byte
// never exceeds 16, so none carries; integers only, so the counts do not depend on the schedule).
__global__ __launch_bounds__(kBlock, 5) void k_area_shadow(SceneDev sc, AreaDev al) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   ItemWalk w(s_walk, t, spill, nullptr, al.counters[1]);
   uint32_t ray = 0, n_occluded = 0;
   auto start = [&](uint32_t item) {
      const float4 r0 = ld_stream(al.rays + 2 * (size_t)item), r1 = ld_stream(al.rays + 2 * (size_t)item + 1);
      ray = __float_as_uint(r0.w);
      const V3 wd = xyz(r1) - xyz(r0);
      const float len = sqrtf(dot3(wd, wd));
      const V3 d = v3(wd.x / len, wd.y / len, wd.z / len);
      const float tmax = len * 0.999f;
      trav_init(t, make_float4(r0.x, r0.y, r0.z, 0.001f), make_float4(d.x, d.y, d.z, tmax), 0.001f, tmax, INFINITY);
   };
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<true, false>(w, sc, occluded)) {
         if (occluded) {
            al.rec_d[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            al.rec_s[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            n_occluded++;
         }
         atomicAdd(al.counts + al.queue[ray / al.samples], occluded ? kAlOccluded : kAlLit);
      }
   }
   wave_add(&al.counters[2], n_occluded);
}

// D and Sp of the pixel in queue slot q: the records summed in sample order, divided by (float)samples, then per channel
// min(x > 0 ? x : 0, max_radiance); one lane walks the samples
__device__ __forceinline__ float area_clamp(float x, float cap) { return fminf(x > 0.0f ? x : 0.0f, cap); }
__global__ __launch_bounds__(kBlock) void k_area_mean(AreaDev al, float4* __restrict__ out_d, float4* __restrict__ out_s) {
   const uint32_t pixels = al.counters[0];
   const float n = (float)al.samples, cap = al.max_radiance;
   for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < pixels; q += gridDim.x * kBlock) {
      const float4* d = al.rec_d + (size_t)q * al.samples;
      const float4* s = al.rec_s + (size_t)q * al.samples;
      V3 sd = xyz(d[0]), sp = xyz(s[0]);
      for (uint32_t k = 1; k < al.samples; k++) sd = sd + xyz(d[k]), sp = sp + xyz(s[k]);
      const uint32_t pix = al.queue[q];
      out_d[pix] = make_float4(area_clamp(sd.x / n, cap), area_clamp(sd.y / n, cap), area_clamp(sd.z / n, cap), 1.0f);
      out_s[pix] = make_float4(area_clamp(sp.x / n, cap), area_clamp(sp.y / n, cap), area_clamp(sp.z / n, cap), 1.0f);
   }
}

// The filter over the tiles of edge_filter.h, D and Sp in one pass over the same taps: the mean over the taps (dx, dy) in [-r, r]^2 that
// cast themselves (a count word that is not 0) and pass the two tests, 1 <= blur_radius <= kAlMaxBlur
constexpr int kAlMaxBlur = 6;
__global__ __launch_bounds__(kBlock) void k_area_filter(HybridDev hd, AreaDev al) {
   using Tile = FilterTile<kAlMaxBlur, 6>;
   __shared__ Tile::Rec s_rec;
   __shared__ Tile::Valid s_valid;
   Tile s_tile{s_rec, s_valid};
   const int r = (int)al.blur_radius;
   const FilterLane me = s_tile.stage(
      hd, r, [&](size_t g) { return al.counts[g] != 0; },
      [&](size_t g, int i) {
         const float4 D = al.mean_d[g], S = al.mean_s[g];
         s_tile.rec[6][i] = D.x, s_tile.rec[7][i] = D.y, s_tile.rec[8][i] = D.z;
         s_tile.rec[9][i] = S.x, s_tile.rec[10][i] = S.y, s_tile.rec[11][i] = S.z;
      });
   if (me.px >= (int)hd.W || me.py >= (int)hd.H || !s_tile.valid[me.centre]) return;  // not a pixel that cast: zeros from the classify
   V3 sd = v3(0.0f, 0.0f, 0.0f), sp = sd;
   const float n = (float)s_tile.taps(
      me.centre, r, r, al.blur_normal_cos, al.blur_plane, [](int, int) { return true; },
      [&](int i) {
         sd = sd + v3(s_tile.rec[6][i], s_tile.rec[7][i], s_tile.rec[8][i]);
         sp = sp + v3(s_tile.rec[9][i], s_tile.rec[10][i], s_tile.rec[11][i]);
      });
   const size_t g = (size_t)me.py * hd.W + me.px;
   al.diffuse[g] = make_float4(sd.x / n, sd.y / n, sd.z / n, 1.0f);
   al.specular[g] = make_float4(sp.x / n, sp.y / n, sp.z / n, 1.0f);
}

// The composite, one lane per pixel that cast: deferred_output.rgb += (((base / PI) Df) + Spf) intensity, base as k_hybrid_deferred forms
// it (frag:61-65); no occlusion, ssao or shadow factor. The gamma table as k_hybrid_deferred has it.
__global__ __launch_bounds__(kBlock) void k_area_composite(SceneDev sc, HybridDev hd, HybridFrameDev fd, AreaDev al) {
   __shared__ float s_gamma[256];
   s_gamma[threadIdx.x] = (float)pow((double)((float)threadIdx.x / 255.0f), (double)2.2f);
   __syncthreads();
   const uint32_t n = hd.W * hd.H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   const float4 Df = al.diffuse[i];
   if (Df.w == 0.0f) return;  // the pixel did not cast
   const float4 Sf = al.specular[i];
   const uchar4 A = hd.alb[i];
   const V3 base = v3(s_gamma[A.x], s_gamma[A.y], s_gamma[A.z]) * area_surface(sc, hd.pbr[i]).bc;
   const V3 bp = v3(base.x / kPiBrdf, base.y / kPiBrdf, base.z / kPiBrdf);
   const V3 add = ((bp * xyz(Df)) + xyz(Sf)) * al.intensity;
   const float4 d = fd.deferred[i];
   fd.deferred[i] = make_float4(d.x + add.x, d.y + add.y, d.z + add.z, d.w);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
// the table from the tree's packets; tab.amax zeroed by the caller, tab.base uploaded; chunks: scan_chunk_count(tab.n) words
uint32_t area_table_chunks(uint32_t n) { return scan_chunk_count(n); }

void launch_area_table(const LaunchCfg& c, const SceneDev& sc, const AreaTableDev& tab, uint32_t* chunks) {
   const dim3 slots((tab.n + kBlock - 1) / kBlock);
   k_area_fill<<<dim3((sc.num_tris + kBlock - 1) / kBlock), kBlock, 0, c.stream>>>(sc.tris, sc.num_tris, tab);
   k_area_weights<<<slots, kBlock, 0, c.stream>>>(tab);
   device_exclusive_scan_u32(tab.cum, tab.n, chunks, tab.total, c.stream);
   k_area_inclusive<<<slots, kBlock, 0, c.stream>>>(tab);
}

void launch_area_sample(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const HybridFrameDev& fd, const AreaDev& al, uint32_t order) {
   const uint32_t n = hd.W * hd.H;
   k_area_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(sc, hd, fd, al);
   const uint64_t items = (uint64_t)n * al.samples;
   const dim3 grid = stream_grid(c, (uint32_t)(items < 0xffffffffull ? items : 0xffffffffull));
   if (order == 0)
      k_area_sample<0><<<grid, kBlock, 0, c.stream>>>(sc, hd, al);
   else
      k_area_sample<1><<<grid, kBlock, 0, c.stream>>>(sc, hd, al);
}

void launch_area_shadow(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const AreaDev& al) {
   const dim3 grid = persistent_grid((uint64_t)hd.W * hd.H * al.samples, c.num_cus * c.shadow_blocks_per_cu);
   k_area_shadow<<<grid, kBlock, 0, c.stream>>>(sc, al);
}

void launch_area_filter(const LaunchCfg& c, const HybridDev& hd, const AreaDev& al) {
   k_area_mean<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(al, al.blur_radius ? al.mean_d : al.diffuse, al.blur_radius ? al.mean_s : al.specular);
   if (!al.blur_radius) return;  // Df = D, Spf = Sp
   k_area_filter<<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, al);
}

void launch_area_composite(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const HybridFrameDev& fd, const AreaDev& al) {
   k_area_composite<<<dim3((hd.W * hd.H + kBlock - 1) / kBlock), kBlock, 0, c.stream>>>(sc, hd, fd, al);
}

}  // namespace uh
