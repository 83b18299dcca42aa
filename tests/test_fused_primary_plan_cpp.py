"""CPU: SamplePlan::fused_primary (product code, csrc/frame_plan.h: where bounce 0 of a sample pass is the one kernel k_primary_shade) as a
stand-alone program (tests/cpp/fused_primary_plan_check.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: each condition of the
plan taken away alone takes it away, over the cross product of its inputs it holds where all of them do and nowhere else, and it never
goes with k_path_fused."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_primary_holds_where_all_of_its_conditions_do(tmp_path):
    exe = str(tmp_path / "fused_primary_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "rust-renderer_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "fused_primary_plan_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FUSED PRIMARY PLAN CHECK OK" in r.stdout and "FAIL" not in r.stdout
