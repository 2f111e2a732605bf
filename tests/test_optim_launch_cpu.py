"""Host-code sanitizer run of the flat optimizers' variant table (csrc/optim_launch.h): a stand-alone program
built with AddressSanitizer + UndefinedBehaviorSanitizer checks opt_variant over the 8 combinations of
(clip, ema, guard) against a table written out literally, what each built wrapper carries for Adam and SGD
(the inner arguments byte for byte, the clip factor or the device 1.0f, ok, the shadow, its decay and flag),
the refusals, and apply_mods on RuleArgs and LayerwiseArgs (tests/native/optim_launch_main.cpp). Only the
header's inline part: no launcher is linked."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.skipif(not os.path.exists(os.path.join(ROCM_INC, "hip", "hip_runtime_api.h")), reason="no ROCm headers")
def test_optim_launch_table_asan_ubsan(tmp_path):
    exe = str(tmp_path / "optim_launch_san")
    src = os.path.join(HERE, "native", "optim_launch_main.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__=1", "-I", os.path.join(HERE, "..", "csrc"),
                    "-I", ROCM_INC, src, "-o", exe], check=True, capture_output=True, timeout=120)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
