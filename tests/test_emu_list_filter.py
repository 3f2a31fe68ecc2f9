"""CPU-only: the list-column filter tests under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_list_filter.py run against
libxgm_emu.so with its small sizes (XGM_EMU_QUICK) and guard pages behind every device buffer: xgm_filter_mark_lists_kernel's head loads at the tail,
its reads of ext (a list column's ext ends with its last document's last ordinal: one word further faults), the divergent walks of lists of very
different lengths inside one wave, and the filtered match and the range search under such a bitmap."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_list_filters_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_list_filter.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "28 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
