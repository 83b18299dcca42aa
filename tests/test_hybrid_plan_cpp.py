"""CPU: the plan of a uh_render_hybrid call (product code, csrc/hybrid_plan.h: which passes run and what they need, or the message of the
first rule the request breaks) as a stand-alone program (tests/cpp/hybrid_plan_check.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer: each of the 39 rules broken alone answers with its code and its whole message, of any two broken rules the
earlier one answers (all 741 pairs), the five capacity rules refuse from W * H = 2^32 / k on and not one pixel sooner, and every field
of an accepted plan is its one-line definition. The header is host code without HIP: it compiles with plain g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_rule_answers_in_the_header_s_order(tmp_path):
    exe = str(tmp_path / "hybrid_plan_check")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "rust-renderer_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "hybrid_plan_check.cpp"), "-o", exe],
        check=True,
    )
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "HYBRID PLAN CHECK OK" in r.stdout and "FAIL" not in r.stdout
