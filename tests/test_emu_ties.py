"""CPU-only: the tied-weight parity tests under the emulated wave kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_ties.py run against
libxgm_emu.so, guard pages behind every device buffer, with its thinned case list (XGM_EMU_QUICK): which of several documents of equal weight a page
holds, through the bodies' sorts, the units' cut-offs, the query-wide thresholds, the merges, the count and frozen kernels and the shard merge of the
C ABI.  Left out: the run under the A/B switches (a process per switch set) and the shard merges fed from torch tensors (they need the device)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_ties_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not kernel_variants and not device_merge",
                        os.path.join("tests", "test_gpu_ties.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "6 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
