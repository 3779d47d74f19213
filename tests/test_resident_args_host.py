"""Host: what a resident-basket call decides before it touches the device (csrc/resident_args.h)
under ASan + UBSan.

tests/cpp/resident_args_test.cpp includes only that header (pure host code, no HIP) and has its own
main: every refusal code of a weighted CSR of id sets, the code that wins when a call is wrong in
two ways, Q == 0 and empty queries, all-zero weights, the factors w_i / W with W summed left to
right bit for bit (and 1 / count without weights), the slot rule, the power of two that holds Kq,
and the host side of hash32 against recorded values. Compiled with g++ -fsanitize=address,undefined
and run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "resident_args_test.cpp")


def test_resident_args_sanitized(tmp_path):
    binary = str(tmp_path / "resident_args_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) >= 70
