"""CPU-only: the live-set, MatchAll, complement and XOR tests under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_filter_all.py
run against libxgm_emu.so with its small sizes (XGM_EMU_QUICK) and guard pages behind every device buffer: xgm_filter_mark_live_kernel's last 16-byte
load and the entry-by-entry read of the group that straddles lastdocid when the doclen section ends the segment, the padded tail of the bitmap it
writes, and xgm_filter_combine_kernel's last group of four words over the cached live set."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_live_set_filters_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_filter_all.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "49 passed in" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
