"""CPU-only: the nested-query edge cases under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_tree_edges.py run against
libxgm_emu.so with guard pages behind every device buffer: the node program of the workgroup match kernel over both widths of the wdf tables, sixteen
groups and fifteen nodes in its per-document arrays, xgm_search_all's listing, the boolean programs of xgm_filter_mark_query_kernel — and the lowering
of xgm_plan.cc, which is host code either way.  The corpus is small as it stands (2 560 documents): XGM_EMU_QUICK changes nothing in that file."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_tree_edges_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_tree_edges.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "8 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
