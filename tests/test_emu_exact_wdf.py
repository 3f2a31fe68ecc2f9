"""CPU-only: the exact wdf = 1 rule of crowded stripes under the emulated wave kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_exact_wdf.py run
against libxgm_emu.so, guard pages behind every device buffer: k_dense_fill's wdf-0 flags, the planes loaded outside the prefilter, the packed plane bits in
the candidate ring and their overflow, the tallies, the first two switch combinations and the units of 8 and of 4 stripes in child processes of the child."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_exact_wdf_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_exact_wdf.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "11 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
