"""Host: the planning of the induced subgraph batches (csrc/subgraph_plan.h) under ASan + UBSan.

tests/cpp/subgraph_plan_test.cpp includes only that header (pure host code, no HIP) and has its own
main: the tier rule gives every source exactly one tier and a table its members fit; the slices of a
source cover its groups once, in order and on group boundaries, and a slice's walk gives every group
the number and the edges the unsliced walk gives it; chunks and walk batches respect their budgets;
the refusals come in their order; the capacity and index-type checks hold at the 2^31 and 2^62
edges without overflow. Compiled with g++ -fsanitize=address,undefined and run as a program of its
own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "subgraph_plan_test.cpp")


def test_subgraph_plan_sanitized(tmp_path):
    binary = str(tmp_path / "subgraph_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 10000
