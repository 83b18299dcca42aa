"""CPU: the path state's address arithmetic (product code, csrc/path_layout.h: what Slot::create allocates and where rec_quad / rec_pair
point) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/cpp/path_layout_check.cpp): for ten
capacities from the 64-path minimum up and both layouts (four quads; the slim state's three quads and a pair), no two planes of a set
overlap, no two records overlap, and every pair lies inside its plane."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quads_and_pairs_stay_inside_their_planes_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "path_layout_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "rust-renderer_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "path_layout_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "PATH LAYOUT CHECK OK" in r.stdout and "MISMATCH" not in r.stdout
