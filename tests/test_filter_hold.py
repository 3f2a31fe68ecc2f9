"""CPU-only, host code only: the reference-counted holder behind the ONE allocation of a filter batch (xapiand_amd/csrc/xgm_filter_hold.h, used by
xgm_filter_build_query_batch and xgm_filter_free) in a stand-alone program of its own — tests/host/filter_hold_main.cc — built with the address and
undefined-behaviour sanitizers: every free order, the last reference frees exactly once, nothing is used after it, nothing leaks; frees from eight
threads at once.  Nothing here is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")


def test_batch_holder_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "filter_hold")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I" + os.path.join(ROOT, "xapiand_amd", "csrc"), os.path.join(ROOT, "tests", "host", "filter_hold_main.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "filter_hold ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
