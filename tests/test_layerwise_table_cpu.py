"""Host-code sanitizer run of the layer-wise block table (csrc/layerwise.h): a stand-alone program built
with AddressSanitizer + UndefinedBehaviorSanitizer builds the table for ragged, gapped, 300-segment and
MNIST segment tables at several chunk sizes and checks coverage, the builder's refusals and the ratio
functions' guards (tests/native/layerwise_table_main.cpp)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_layerwise_table_asan_ubsan(tmp_path):
    exe = str(tmp_path / "layerwise_table_san")
    src = os.path.join(HERE, "native", "layerwise_table_main.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True, capture_output=True, timeout=120)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
