"""Host check of the float16 / bfloat16 -> float32 conversions the one-kernel SAGE layer applies to a 16-bit feature table
(cugraph-gnn_amd/csrc/wg_x16.hpp): tests/host/x16_convert_check.cpp, a stand-alone program, runs the kernel's own functions
compiled for the host over all 65536 bit patterns against ``__half2float``, a 16-bit shift and a bit-level decoder, by bits.
No GPU: the program is compiled host-only and starts no HIP runtime call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_conversions_agree_on_every_bit_pattern(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found at %s: the conversions cannot be checked" % HIPCC)
    exe = tmp_path / "x16_convert_check"
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "cugraph-gnn_amd", "csrc"), os.path.join(ROOT, "tests", "host", "x16_convert_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok (65536 patterns" in out.stdout
