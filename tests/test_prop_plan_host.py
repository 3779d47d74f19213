"""Host: the planning of the transposed feature propagation (csrc/prop_plan.h) under ASan + UBSan.

tests/cpp/prop_plan_test.cpp includes only that header (pure host code, no HIP) and has its own
main: the key ranges partition the keys, hold at most E postings unless they are one key, and are
maximal; the chunk tasks cover every posting once, in order, in chunks of PPR_PROP_CHUNK; partial
rows and fold tasks line up; the column blocks respect their budget; and the weight rule, W == 0
included. Compiled with g++ -fsanitize=address,undefined and run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "prop_plan_test.cpp")


def test_prop_plan_sanitized(tmp_path):
    binary = str(tmp_path / "prop_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 1000
