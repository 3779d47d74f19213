"""Host: when a recorded merge plan may be replayed (csrc/replay_rule.h) under ASan + UBSan.

tests/cpp/replay_rule_test.cpp includes only that header (pure host code, no HIP) and has its own
main: an unchanged length-change counter replays; a moved counter, another list range or partition,
an init in between (a drop) and each disabling knob (PPR_REPLAY=0, a sharded plan, PPR_WAVE_BY_D,
PPR_SV_SEEDLESS, a hot set) do not. Compiled with g++ -fsanitize=address,undefined and run as a
program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "replay_rule_test.cpp")


def test_replay_rule_sanitized(tmp_path):
    binary = str(tmp_path / "replay_rule_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", binary], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert p.returncode == 0, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[0] == "ok" and int(out[1]) > 30
