"""The trace arena's slot match (halo2_rsa_amd/csrc/h2r_arena_match.hpp) as a stand-alone host program under the address and
undefined-behaviour sanitizers: which record launches lie on record slots of a registered region (tests/cpp/test_arena_match.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_slot_match_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_arena_match")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "halo2_rsa_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_arena_match.cpp"),
                           "-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ARENA_MATCH_OK" in out.stdout
