"""CPU: the blocked texture layout (product code, csrc/texture_layout.h: the repack of uh_add_texture_rgba8 and the address function
of sample_texture_pre) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/cpp/texture_layout_check.cpp):
for ten sizes from 1x1 to 64x64 and both block geometries (8x4 and 4x4 texels), every footprint of [-3w, 3w) x [-3h, 3h) reads the
row-major source's texels through mirror_index, no address leaves the allocation, and a size whose blocked texel count exceeds 2^32
is refused with UH_ERR_CAPACITY."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blocked_layout_reads_the_source_texels_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "texture_layout_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "rust-renderer_amd", "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "texture_layout_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "TEXTURE LAYOUT CHECK OK" in r.stdout and "MISMATCH" not in r.stdout
    assert "footprints checked: 175104 (8x4) + 175104 (4x4)" in r.stdout  # the sum over the ten sizes of 6w * 6h
