// denoise_host.cpp — the denoiser through the C++ host mirror (include/utopian_host.hpp): Renderer::add_model, Raytracing::initialize,
// then two rounds of one path-traced frame (total_samples = samples_per_frame, view.time 0.125 apart), the hybrid G-buffer and
// Renderer::denoise - the first with the default params, the second with the blob's view as it is (a camera at rest: the blob carries
// its own projection * view as prev_frame_projection_view) - and read_denoised of all six images after the second.
// The scene arrives as a blob written by tests/hybrid_util.py; the test renders the same bytes through the ctypes path and compares.
//   usage: denoise_host <scene.blob> <out.bin>
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
      ViewUniformData view = rd<ViewUniformData>(f);
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
      const UhDenoiseParams params = Renderer::default_denoise_params();
      for (int round = 0; round < 2; round++) {
         renderer.check(uh_render_frame(renderer.handle(), &view, UH_PASS_REFERENCE_PT), "render_frame");
         renderer.render_hybrid(view, UH_HYBRID_GBUFFER);
         if (round == 0) renderer.denoise(view, params);
         else renderer.denoise(view);
         view.time += 0.125f;
      }
      std::ofstream out(argv[2], std::ios::binary);
      for (int which = UH_DENOISE_COLOR; which <= UH_DENOISE_VARIANCE; which++) {
         const std::vector<uint8_t> img = renderer.read_denoised(which);
         out.write(reinterpret_cast<const char*>(img.data()), (std::streamsize)img.size());
      }
      const UhDenoiseStats s = renderer.denoise_stats();
      std::printf("geometry %u history %u\n", s.geometry_pixels, s.history_pixels);
      return 0;
   } catch (const Error& e) {
      std::fprintf(stderr, "utopian::Error %d: %s\n", e.status, e.what());
      return e.status == UH_ERR_NO_DEVICE ? 3 : 1;
   } catch (const std::exception& e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
}
