"""CPU-only: the posting format's edges under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_format_edges.py run against
libxgm_emu.so, guard pages behind every device buffer: k_dense_fill / k_flat_fill / k_narrow_doclen and the block decoders at gap and wdf widths 0 and
maximal, the one-word look-ahead of the bit extraction and the two words staged past a block's payload where that payload ends the word section, wdf 254 /
255, the position lists at 65 535 / 65 536, lastdocid at a stripe seam.  The processes per A/B switch stay on the device."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_format_edges_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_format_edges.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and re.search(r"\b21 passed, 7 skipped", r.stdout), r.stdout[-4000:] + r.stderr[-2000:]
