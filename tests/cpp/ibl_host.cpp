// ibl_host.cpp — the IBL maps through the C++ host mirror (include/utopian_host.hpp): the scene blob of tests/test_hybrid_cpp.py (its
// view with ibl_enabled and cubemap_enabled set), one render_hybrid with UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT, read_environment of
// the irradiance cube's face 2, read_hybrid of the present image and the environment stats. tests/test_gpu_ibl.py renders the same
// bytes through the ctypes path and compares.
//   usage: ibl_host <scene.blob> <out.bin>
#include <cstdio>
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
   if (argc < 3) {
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
      renderer.render_hybrid(view, UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT);
      std::ofstream out(argv[2], std::ios::binary);
      const std::vector<float> irr = renderer.read_environment(UH_ENV_IRRADIANCE, 2, 0);
      out.write(reinterpret_cast<const char*>(irr.data()), (std::streamsize)(irr.size() * sizeof(float)));
      const std::vector<uint8_t> img = renderer.read_hybrid(UH_HYBRID_PRESENT_OUTPUT);
      out.write(reinterpret_cast<const char*>(img.data()), (std::streamsize)img.size());
      const UhEnvironmentStats s = renderer.environment_stats();
      std::printf("builds %u\n", s.builds);
      return 0;
   } catch (const Error& e) {
      std::fprintf(stderr, "utopian::Error %d: %s\n", e.status, e.what());
      return e.status == UH_ERR_NO_DEVICE ? 3 : 1;
   } catch (const std::exception& e) {
      std::fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
}
