"""CPU-only: the two-stage bitmap loads of xgm_dense_unit under the emulated wave kernels (tests/emu, see tests/test_emu.py) — the whole of
tests/test_gpu_staged_bitmaps.py run against libxgm_emu.so, guard pages behind every device buffer: the masked loads of plan terms 2 and 3, the pipeline's
prologue and end for units of 1, 2 and 3 qualifying stripes, the tallies, every switch combination and the units of 8 and of 4 stripes (with and without the
switch) in child processes of the child."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_staged_bitmaps_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_staged_bitmaps.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "17 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
