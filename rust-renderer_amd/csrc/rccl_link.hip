// rccl_link.hip — one process per GPU: the communicator a context is attached to (uh_rccl_attach), the reservoir bands' exchange over
// it and the gather of a tile-partitioned frame (uh_rccl_gather_tiles). librccl is opened at run time (types from its header, no link
// dependency): a process that never attaches needs no RCCL at all, and one that has torch's copy loaded gets that same copy (same
// soname). The partitions themselves and the pack / compose this file enqueues are partition.hip.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only
#include <dlfcn.h>

#include <cstring>
#include <string>

#include "context_internal.h"
#include "context_state.h"
#include "utopian_hip.h"

struct __attribute__((visibility("hidden"))) RcclLink {
   ncclComm_t comm = nullptr;
   uint32_t rank = 0, world = 1;
};

namespace {
// the entry points used, in the order of RcclApi's pointers behind `so`; the last two may be absent
#define UH_RCCL_NAMES(X) X(GetUniqueId) X(CommInitRank) X(CommDestroy) X(AllGather) X(Send) X(Recv) X(GroupStart) X(GroupEnd) X(CommCount) X(GetErrorString)
struct RcclApi {
   void* so = nullptr;
#define X(name) decltype(&nccl##name) name = nullptr;
   UH_RCCL_NAMES(X)
#undef X
   std::string why;
};
RcclApi* rccl_api() {
   static RcclApi api;
   static bool tried = false;
   if (tried) return &api;
   tried = true;
   for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.so = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.so) break;
   }
   if (!api.so) {
      api.why = std::string("librccl not found: ") + (dlerror() ? dlerror() : "");
      return &api;
   }
#define X(name) api.name = (decltype(api.name))dlsym(api.so, "nccl" #name);
   UH_RCCL_NAMES(X)
#undef X
   if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather || !api.Send || !api.Recv || !api.GroupStart || !api.GroupEnd) {
      api.why = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd";
      api.so = nullptr;
   }
   return &api;
}
// UhRestirExchangeFn: in-place all-gather of the bands, enqueued on the reservoir stream
int rccl_exchange(void* user, void* stream, void* base, uint64_t band_bytes, uint32_t rank, uint32_t) {
   RcclLink* l = (RcclLink*)user;
   return (int)rccl_api()->AllGather((const char*)base + (size_t)rank * band_bytes, base, (size_t)band_bytes, ncclInt8, l->comm, (hipStream_t)stream);
}
}  // namespace

void uh_ctx::Bands::destroy() {
   if (!link) return;
   if (link->comm) (void)rccl_api()->CommDestroy(link->comm);
   delete link;
   link = nullptr;
   if (exchange == rccl_exchange) {
      exchange = nullptr;
      user = nullptr;
   }
}

extern "C" {

int uh_rccl_unique_id(uint8_t out_id[128]) {
   static_assert(sizeof(ncclUniqueId) == 128, "the C ABI hands the id over as 128 bytes");
   if (!out_id) return UH_ERR_INVALID_ARGUMENT;
   RcclApi* api = rccl_api();
   if (!api->so) return UH_ERR_HIP;
   ncclUniqueId id;
   if (api->GetUniqueId(&id) != ncclSuccess) return UH_ERR_HIP;
   memcpy(out_id, &id, 128);
   return UH_OK;
}

int uh_rccl_attach(uh_ctx* c, uint32_t rank, uint32_t world, const uint8_t id[128]) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!id || world == 0 || rank >= world) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_rccl_attach: need an id and rank < world");
   RcclApi* api = rccl_api();
   if (!api->so) return fail(c, UH_ERR_HIP, "uh_rccl_attach: " + api->why);
   HIP_TRY(c, hipSetDevice(c->device));
   uh_rccl_detach(c);
   RcclLink* l = new RcclLink();
   ncclUniqueId nid;
   memcpy(&nid, id, 128);
   const ncclResult_t r = api->CommInitRank(&l->comm, (int)world, nid, (int)rank);
   if (r != ncclSuccess) {
      delete l;
      return fail(c, UH_ERR_HIP, std::string("ncclCommInitRank: ") + (api->GetErrorString ? api->GetErrorString(r) : "failed"));
   }
   l->rank = rank;
   l->world = world;
   c->bands.link = l;
   return uh_set_restir_partition(c, rank, world, rccl_exchange, l);
}

int uh_rccl_detach(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!c->bands.link) return UH_OK;
   (void)hipSetDevice(c->device);
   (void)sync_all(c);
   c->bands.destroy();
   return UH_OK;
}

int uh_rccl_comm_count(uh_ctx* c, uint32_t* out_ranks) {
   if (!c || !out_ranks) return UH_ERR_INVALID_ARGUMENT;
   *out_ranks = 0;
   RcclLink* l = c->bands.link;
   if (!l) return UH_OK;
   int n = 0;
   if (!rccl_api()->CommCount || rccl_api()->CommCount(l->comm, &n) != ncclSuccess) return fail(c, UH_ERR_HIP, "ncclCommCount failed");
   *out_ranks = (uint32_t)n;
   return UH_OK;
}

// The ONE collective of the path tracer's data path. Every rank packs its tiles of pt_accumulation_image and sends
// them to `root` over the communicator uh_rccl_attach made (grouped ncclSend / ncclRecv: the peers' buffers arrive on distinct xGMI
// links at once; the root's own tiles take the same way, a local copy); the root scatters them and recomputes pt_output_image in one
// launch (renderers/mod.rs:199-214,354-358: the two images a single device holds). All of it on the context's stream, behind the
// frames in flight; the call returns at once and the next uh_read_* / uh_synchronize waits.
int uh_rccl_gather_tiles(uh_ctx* c, uint32_t root, uint32_t total_samples, uint32_t accumulation_limit) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   RcclLink* l = c->bands.link;
   uh_ctx::Tiles& t = c->tiles;
   if (!l) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_rccl_gather_tiles: no communicator attached (uh_rccl_attach)");
   if (t.world != l->world || t.rank != l->rank)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_rccl_gather_tiles: uh_set_tile_partition(rank, world) must be the communicator's rank and size");
   if (root >= l->world) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_rccl_gather_tiles: root >= world");
   HIP_TRY(c, hipSetDevice(c->device));
   const uint64_t stride = max_pack_pixels(c);
   const bool is_root = l->rank == root;
   if (t.send.n < stride || (is_root && t.recv.n < stride * l->world)) {
      if (int st = sync_all(c)) return st;  // (first call, or another partition: the old buffers may still be read)
      HIP_TRY(c, t.send.alloc(stride ? stride : 1));
      if (is_root) HIP_TRY(c, t.recv.alloc((stride ? stride : 1) * l->world));
   }
   if (int st = uhi_enqueue_pack_tiles(c, t.send.p, nullptr)) return st;
   RcclApi* api = rccl_api();
   ncclResult_t r = api->GroupStart();
   uint64_t mine = 0;
   uh_tile_pack_count(c, l->rank, &mine);
   if (r == ncclSuccess && mine) r = api->Send(t.send.p, (size_t)mine * 4, ncclFloat, (int)root, l->comm, c->stream);
   if (is_root)
      for (uint32_t k = 0; k < l->world && r == ncclSuccess; k++) {
         uint64_t n = 0;
         uh_tile_pack_count(c, k, &n);
         if (n) r = api->Recv(t.recv.p + (size_t)k * stride, (size_t)n * 4, ncclFloat, (int)k, l->comm, c->stream);
      }
   const ncclResult_t e = api->GroupEnd();
   if (r == ncclSuccess) r = e;
   if (r != ncclSuccess) return fail(c, UH_ERR_HIP, std::string("uh_rccl_gather_tiles: ") + (api->GetErrorString ? api->GetErrorString(r) : "RCCL error"));
   if (is_root) return uhi_enqueue_compose_tiles(c, t.recv.p, stride, total_samples, accumulation_limit, nullptr, 0);
   return mark_composed(c);
}

}  // extern "C"
