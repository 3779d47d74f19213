"""Host: the planning of the node-pair scores (csrc/pairs_plan.h) under ASan + UBSan.

tests/cpp/pairs_plan_test.cpp includes only that header (pure host code, no HIP) and has its own
main: the refusals come in their order; every group gets exactly one tier; the tasks of a split group
cover its candidates once and in order; chunks respect their budgets and cover the call; the size
checks hold at 2^31 - 1 and 2^62 without overflow; the limb sums of the wave reduction equal
unsigned __int128 sums of random values of up to 95 bits in random groupings (12 000 cases); the byte
accounting gives the header's figures on hand-made groups. Compiled with g++
-fsanitize=address,undefined and run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "pairs_plan_test.cpp")


def test_pairs_plan_sanitized(tmp_path):
    binary = str(tmp_path / "pairs_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 30000
