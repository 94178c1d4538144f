"""CPU: the functions the setup kernels share with the host (csrc/h2r_setup.hpp) compiled with
-Xarch_host -fsanitize=address,undefined (the host pass alone is instrumented; nothing is built for or run on a device) into the stand-alone
program tests/cpp/test_setup_shared.cpp (host code only, its own main, no library) and run over exact-size heap buffers: any access past the
table or undefined shift in the window bases, the digit walk, the scalar families or the G2 multiplication aborts it."""
import os
import subprocess

from halo2_rsa_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_setup_functions_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "test_setup_shared")
    subprocess.check_call([_build.hipcc_path(), "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + _build.CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_setup_shared.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "SETUP_SHARED_OK 2 representations" in out.stdout
