"""The prover stages' buffer arithmetic (halo2_rsa_amd/csrc/h2r_stage_args.hpp) as a stand-alone host program under the address and
undefined-behaviour sanitizers: alignment, column blocks, overlap and launch slices against the formulas every stage export used to
spell out for itself, the multi-slice launches included (tests/cpp/test_stage_args.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_args_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_stage_args")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1",
                           "-I" + os.path.join(ROOT, "halo2_rsa_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_stage_args.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "STAGE_ARGS_OK" in out.stdout
