"""CPU-only: the wdf summary and its users under the emulated wave kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_wdf_summary.py run against
libxgm_emu.so, guard pages behind every device buffer: k_dense_fill's summary words, xgm_dense_unit's masked byte probes, xgm_flat_unit's bit screen and
its survivors' byte, the tallies, and the first three switch combinations in child processes of the child.  The emulator rendezvouses a wave operation per
call site, so it also shows a wave operation that only part of a wave reaches."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_wdf_summary_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_wdf_summary.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "9 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
