"""Host: the planning of the sweep cuts (csrc/sweep_plan.h) under ASan + UBSan.

tests/cpp/sweep_plan_test.cpp includes only that header (pure host code, no HIP) and has its own
main: the tier rule gives every source exactly one tier and a table its members fit; the slices of
a source cover [0, W) once and in order and a batch holds at most its budget of histogram rows; the
chunks respect their budgets; the refusals come in their order; and the exact comparison of two
ratios agrees with __int128 on random and extreme pairs, denominators near 2^62 included. Compiled
with g++ -fsanitize=address,undefined and run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "sweep_plan_test.cpp")


def test_sweep_plan_sanitized(tmp_path):
    binary = str(tmp_path / "sweep_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 100000
