"""CPU: the tile partition's owner rule (product code, csrc/tile_partition.h: what uh_set_tile_partition, uh_tile_pack_count, the pack /
compose kernels and owns_pixel compute with) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
(tests/cpp/tile_partition_check.cpp): for frames of 1, 7, 64, 65 and 130 pixels a side, tiles of 1, 8, 64 and 100, worlds of 1, 2, 3 and
8 and one world larger than the tile count, the header's closed forms agree with the partition dealt out tile by tile and painted
pixel by pixel, every pixel has exactly one owner, and a rank's in-frame packed positions are exactly its owned-pixel list."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_rule_and_packed_map_against_plain_loops_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tile_partition_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "rust-renderer_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tile_partition_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "TILE PARTITION CHECK OK" in r.stdout and "MISMATCH" not in r.stdout
