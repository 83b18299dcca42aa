#!/usr/bin/env python3
"""A measurement library: the csrc file that holds k_path_fused compiled with extra -D switches, linked with the default build's other
objects. Its use is the instrumented build of tools/fused_phase_profile.py (UH_FUSED_PROFILE, the only switch the kernels read):
  python tools/build_variant.py prof -DUH_FUSED_PROFILE   ->  rust-renderer_amd/libuh_prof.so   (UTOPIAN_HIP_LIB takes it)
With --source PATH the file at PATH - an edited copy of a csrc file, kept outside the tree under that file's name - is compiled in the
place of its namesake: a library with a planted fault, to show that a test fails on it (tests/test_gpu_sun_grid_builders.py):
  python tools/build_variant.py halfpad --source /tmp/variants/sun_grid_build.hip"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rust_renderer_amd as rr  # noqa: E402

pkg = os.path.dirname(rr.__file__) if not rr.__file__.endswith("rust_renderer_amd.py") else os.path.join(ROOT, "rust-renderer_amd")
sys.path.insert(0, pkg)
import build as b  # noqa: E402

name, flags = sys.argv[1], sys.argv[2:]
b.build_library()
if "--source" in flags:
    path = os.path.abspath(flags.pop(flags.index("--source") + 1))
    flags.remove("--source")
    src = os.path.basename(path)
    assert os.path.exists(os.path.join(b.CSRC, src)), "%s replaces no file of csrc" % src
else:
    src = next(f for f in sorted(os.listdir(b.CSRC)) if f.endswith(".hip") and "void k_path_fused(" in open(os.path.join(b.CSRC, f)).read())
    path = os.path.join(b.CSRC, src)
obj = os.path.join(b.OBJ_DIR, "variant_%s.o" % name)
subprocess.run(["hipcc"] + b.HIPCC_FLAGS + flags + ["-I", os.path.join(ROOT, "include"), "-I", b.CSRC, "-c", path, "-o", obj], check=True)
others = [os.path.join(b.OBJ_DIR, f) for f in os.listdir(b.OBJ_DIR) if f.endswith(".o") and f != src + ".o" and not f.startswith("variant_")]
lib = os.path.join(pkg, "libuh_%s.so" % name)
subprocess.run(["hipcc", "-shared", "-fPIC", "--offload-arch=gfx950", "-pthread", "-o", lib, obj] + others, check=True)
print(lib)
