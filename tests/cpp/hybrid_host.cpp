// hybrid_host.cpp — the hybrid graph through the C++ host mirror (include/utopian_host.hpp): Renderer::add_model,
// Raytracing::initialize, then per mode
//   passes  render_hybrid with UH_HYBRID_GBUFFER, then with all three ray-traced passes; read_hybrid of the six images; the hybrid stats
//   frame   render_hybrid with UH_HYBRID_FRAME; read_hybrid of the SSAO, deferred and present images; the frame stats
//   ibl     render_hybrid with UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT (the blob's view sets ibl_enabled and cubemap_enabled);
//           read_environment of the irradiance cube's face 2, read_hybrid of the present image; the environment stats
// The scene arrives as a blob written by tests/hybrid_util.py; the tests render the same bytes through the ctypes path and compare.
//   usage: hybrid_host <passes|frame|ibl> <scene.blob> <out.bin>
#include <cstdio>
#include <string>
#include <fstream>

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
   const std::string mode = argc == 4 ? argv[1] : "";
   if (mode != "passes" && mode != "frame" && mode != "ibl") {
      std::fprintf(stderr, "usage: %s passes|frame|ibl scene.blob out.bin\n", argv[0]);
      return 2;
   }
   try {
      std::ifstream f(argv[2], std::ios::binary);
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
      std::ofstream out(argv[3], std::ios::binary);
      const auto write = [&out](const void* p, size_t bytes) { out.write(static_cast<const char*>(p), (std::streamsize)bytes); };
      if (mode == "passes") {
         renderer.render_hybrid(view, UH_HYBRID_GBUFFER);
         renderer.render_hybrid(view);
         for (int which = UH_HYBRID_POSITION; which <= UH_HYBRID_REFLECTIONS; which++) {
            const std::vector<uint8_t> img = renderer.read_hybrid(which);
            write(img.data(), img.size());
         }
         const UhHybridStats s = renderer.hybrid_stats();
         std::printf("rays %llu %llu %llu metal %u\n", (unsigned long long)s.rays[0], (unsigned long long)s.rays[1], (unsigned long long)s.rays[2], s.reflection_pixels);
      } else if (mode == "frame") {
         renderer.render_hybrid(view, UH_HYBRID_FRAME);
         for (int which = UH_HYBRID_SSAO_IMAGE; which <= UH_HYBRID_PRESENT_OUTPUT; which++) {
            const std::vector<uint8_t> img = renderer.read_hybrid(which);
            write(img.data(), img.size());
         }
         const UhHybridFrameStats s = renderer.hybrid_frame_stats();
         std::printf("sky %u lights %u\n", s.sky_pixels, s.lights);
      } else {
         renderer.render_hybrid(view, UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT);
         const std::vector<float> irr = renderer.read_environment(UH_ENV_IRRADIANCE, 2, 0);
         write(irr.data(), irr.size() * sizeof(float));
         const std::vector<uint8_t> img = renderer.read_hybrid(UH_HYBRID_PRESENT_OUTPUT);
         write(img.data(), img.size());
         const UhEnvironmentStats s = renderer.environment_stats();
         std::printf("builds %u\n", s.builds);
      }
      return 0;
   } catch (const Error& e) {
      std::fprintf(stderr, "utopian::Error %d: %s\n", e.status, e.what());
      return e.status == UH_ERR_NO_DEVICE ? 3 : 1;
   } catch (const std::exception& e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
}
