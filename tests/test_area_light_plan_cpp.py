"""CPU: the area-light pass's row of the plan of a uh_render_hybrid call (product code, csrc/hybrid_plan.h) as a stand-alone program
(tests/cpp/area_light_plan_check.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: its four rules with their codes and whole
messages in their order, their place behind the glass pass's rules, no rule on ibl_enabled, the capacity rule at 2^28 pixels and not one
sooner, and the requests without the bit accepted as before."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_area_light_rules_answer_behind_the_glass_rules(tmp_path):
    exe = str(tmp_path / "area_light_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "rust-renderer_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "area_light_plan_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "AREA LIGHT PLAN CHECK OK" in r.stdout and "FAIL" not in r.stdout
