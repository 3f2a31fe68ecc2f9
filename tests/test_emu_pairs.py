"""CPU-only: the pair spy's tests under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_pairs.py run against libxgm_emu.so
with its fewer calls (XGM_EMU_QUICK) and guard pages behind every device buffer: a tail read of a column or of the bitmap past lastdocid, a counter
beyond P, a slot beyond S or a pair placed beyond the records' buffer ends the run; the scans, the probing and the three paths run as they are, the child processes
of the forced table (XGM_PAIRS_DENSE_MAX=0) and of the capped grids (XGM_RANGE_MAX_GRID) included."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_pair_counts_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_pairs.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "15 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
