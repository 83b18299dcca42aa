// gbuffer_raster_host.cpp — the hybrid graph's rasterised G-buffer through the C++ host mirror (include/utopian_host.hpp):
// Renderer::add_model, Raytracing::initialize, render_hybrid with UH_HYBRID_GBUFFER | UH_HYBRID_GBUFFER_RASTER, then read_hybrid of the
// four targets, the pass's depth buffer and its visibility, and the pass's stats. The scene arrives as the blob tests/hybrid_util.py
// writes; the test renders the same bytes through the ctypes path and compares.
//   usage: gbuffer_raster_host <scene.blob> <out.bin>
#include <cstdio>
#include <fstream>
#include <string>

#include "utopian_host.hpp"

using namespace utopian;

template <typename T>
static T rd(std::ifstream& f) {
   T v;
   f.read(reinterpret_cast<char*>(&v), sizeof(T));
   if (!f) throw std::runtime_error("truncated scene blob");
   return v;
}

int main(int argc, char** argv) {
   if (argc != 3) {
      std::fprintf(stderr, "usage: %s scene.blob out.bin\n", argv[0]);
      return 2;
   }
   try {
      std::ifstream f(argv[1], std::ios::binary);
      if (!f) throw std::runtime_error("cannot open scene blob");
      if (rd<uint32_t>(f) != 0x44594855u) throw std::runtime_error("bad magic");
      const uint32_t W = rd<uint32_t>(f), H = rd<uint32_t>(f);
      const ViewUniformData view = rd<ViewUniformData>(f);
      Renderer renderer(0, W, H);  // throws utopian::Error(UH_ERR_NO_DEVICE) when there is no GPU
      renderer.initialize();
      Model model;
      const uint32_t nmesh = rd<uint32_t>(f);
      for (uint32_t i = 0; i < nmesh; i++) {
         Mesh mesh;
         const uint32_t nv = rd<uint32_t>(f), ni = rd<uint32_t>(f);
         mesh.material.material_type = (MaterialType)rd<uint32_t>(f);
         for (float& c : mesh.material.base_color_factor) c = rd<float>(f);
         mesh.primitive.vertices.resize(nv);
         mesh.primitive.indices.resize(ni);
         f.read(reinterpret_cast<char*>(mesh.primitive.vertices.data()), (std::streamsize)(nv * sizeof(Vertex)));
         f.read(reinterpret_cast<char*>(mesh.primitive.indices.data()), (std::streamsize)(ni * sizeof(uint32_t)));
         if (!f) throw std::runtime_error("truncated mesh");
         model.meshes.push_back(std::move(mesh));
      }
      renderer.add_model(std::move(model), Mat4::identity());
      renderer.initialize_raytracing();
      std::ofstream out(argv[2], std::ios::binary);
      renderer.render_hybrid(view, UH_HYBRID_GBUFFER | UH_HYBRID_GBUFFER_RASTER);
      for (int which : {(int)UH_HYBRID_POSITION, (int)UH_HYBRID_NORMAL, (int)UH_HYBRID_ALBEDO, (int)UH_HYBRID_PBR, (int)UH_HYBRID_GBUFFER_DEPTH,
                        (int)UH_HYBRID_GBUFFER_VISIBILITY}) {
         const std::vector<uint8_t> img = renderer.read_hybrid(which);
         out.write(reinterpret_cast<const char*>(img.data()), (std::streamsize)img.size());
      }
      const UhGbufferRasterStats s = renderer.gbuffer_raster_stats();
      std::printf("renders %u pieces %u covered %u\n", s.renders, s.pieces, s.covered_pixels);
      return 0;
   } catch (const Error& e) {
      std::fprintf(stderr, "utopian::Error %d: %s\n", e.status, e.what());
      return e.status == UH_ERR_NO_DEVICE ? 3 : 1;
   } catch (const std::exception& e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
}
