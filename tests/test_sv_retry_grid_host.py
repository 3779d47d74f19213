"""Host: the sieve's retry-grid rule (csrc/sv_plan.h sv_retry_grid) under ASan + UBSan.

tests/cpp/sv_retry_grid_test.cpp includes only that header (pure host code, no HIP) and has its own
main: the whole class at a partition's first sieved update, 2 * prev + 64 capped at the class later,
no launch after two updates without an overflow, and the PPR_SV_RETRY_GRID overrides (legacy, full,
a fixed N). Compiled with g++ -fsanitize=address,undefined and run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "sv_retry_grid_test.cpp")


def test_sv_retry_grid_rule_sanitized(tmp_path):
    binary = str(tmp_path / "sv_retry_grid_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 40
