"""CPU-only: the positional filter's edge cases under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_positional_edges.py run
against libxgm_emu.so with guard pages behind every device buffer: the three stagings of the positions (xgm_dense_body.inc, xgm_flat_body.inc, the wave
kernel's own in xgm_kernels.hip) with their second 16-byte load, the wide layout and the serial copy, the predicates of xgm_posfilter.h on LDS data and
straight from memory, the workgroup kernel's.  The last list of the positions section is a 4-byte list of 254 entries: the serial copy's partial chunk and
the 16-byte loads of the short lists before it end in XGM_POS_PAD, and one byte further is a guard page.  The corpus is small as it stands (3 839 documents);
XGM_EMU_QUICK leaves out the one-process-per-switch runs and all but one pass of the cases asked alone."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_positional_edges_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_positional_edges.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "5 passed, 6 skipped" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
