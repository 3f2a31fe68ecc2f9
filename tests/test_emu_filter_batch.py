"""CPU-only: the batched query-filter tests under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_filter_batch.py run against
libxgm_emu.so with its small sizes (XGM_EMU_QUICK) and guard pages behind every device buffer: xgm_filter_mark_query_batch_kernel's 16-byte loads of
the base filter in the last unit (6 documents of 8192: most lanes lie beyond the padded bitmap), its stores into the LAST bitmap of the batch's one
allocation, and the last entry of the program array, which ends where the scratch's allocation ends.  The two children of the stride-loop test run
emulated as well; the three per-switch children are skipped, as in tests/test_emu_filter_query.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_batched_query_filters_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_filter_batch.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "23 passed, 3 skipped" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
