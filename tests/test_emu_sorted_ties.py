"""CPU-only: sorted and collapsed searches at tied keys and buffer edges under the emulated kernels (tests/emu, see tests/test_emu.py) —
tests/test_gpu_sorted_ties.py run against libxgm_emu.so, guard pages behind every device buffer, with its thinned case list (XGM_EMU_QUICK): at least one
case per buffer size and sort mode, and a collapse at k = 1024, the only size that reaches collapse_prune's drop[4 .. 7].  Left out: the run with one unit per
query (a process of its own).  And, without any kernel: the conditions on the inputs of the FULL case list, proved from the oracle alone."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_input_conditions_of_the_full_case_list(built):
    """Listed equals computed for every sort case, three quarters of them boundary cases, a boundary class in 6 of 8 stripes for every mode, all three buffer
    sizes; the collapse cases' four conditions; the thinned list keeps every buffer size under every mode and the collapse at k = 1024."""
    import test_gpu_sorted_ties as T
    w = T.World()
    try:
        T.check_sort_inputs(w, T.sort_cases(False), quick=False)
        T.check_collapse_inputs(w, T.collapse_cases(False), quick=False)
        T.check_sort_inputs(w, T.sort_cases(True), quick=True)
    finally:
        w.close()
    classes = lambda cases: {(T.cap_of(*T.PAGES[c[1]]), c[2]) for c in cases}
    assert classes(T.sort_cases(True)) == classes(T.sort_cases(False)) == {(cap, m) for cap in (512, 1024, 2048) for m in ("V", "VR", "RV")}
    assert any(T.cap_of(*T.PAGES[c[1]]) == 2048 and c[5] == "ckey" for c in T.collapse_cases(True))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")
def test_sorted_ties_under_emulation(built):
    import test_gpu_sorted_ties as T
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    limit = 120 + 3 * 0.25 * T.quick_searches()                      # about 0.25 s a search where the machine is busy, with a factor of 3; the corpora on top
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not one_unit_per_query",
                        os.path.join("tests", "test_gpu_sorted_ties.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0 and "7 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
