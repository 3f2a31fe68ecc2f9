"""CPU-only: the replay kernels on crafted lists under the emulated kernels (tests/emu, see tests/test_emu.py) — tests/test_gpu_replay_edges.py run against
libxgm_emu.so, guard pages behind every device buffer, with its thinned case list (XGM_EMU_QUICK): every seam position of the workgroup kernel as an event and
as the heap's making, every branch of the freeze, S in (4, 17) and K in (1, 65, 129) of the parallel formulation with both seams, the ring's second lap and an
empty tail.  And, without any kernel: the conditions on the inputs of the FULL case list, proved from the lists and the Python reference's trace alone, and
that reference pinned to the two host restatements that are themselves pinned to the compiled reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_input_conditions_of_the_full_case_list(built):
    """Every named situation occurs in the full list and — those the issue keeps — in the thinned one; no case is skipped: the lists of the test functions are
    the lists checked here, every test function runs all of its own, and none carries a skip."""
    import test_gpu_replay_edges as T
    full, quick = T.all_cases(False), T.all_cases(True)
    T.check_replay_inputs(full, quick=False)
    T.check_replay_inputs(quick, quick=True)
    assert {c.name for c in quick} <= {c.name for c in full}                   # thinned, not different
    parts = (T.serial_count_cases, T.placed_cases, T.lone_cases, T.pivot_cases, T.frozen_cases, T.parallel_cases)
    assert sum(len(p(False)) for p in parts) == len(full) and all(p(q) for p in parts for q in (False, True))
    src = open(T.__file__).read()
    assert "pytest.skip" not in src and "mark.skip" not in src and "xfail" not in src
    for p in parts:                                                            # every part is what some test function runs
        assert "%s()" % p.__name__ in src.split("def test_serial_count_patterns")[1], p.__name__


def test_reference_counts_what_the_host_restatement_counts(built):
    """protomset()'s known_matching_docs = xgm_known_matching_docs (pinned to the compiled reference by tests/test_oracle_vs_reference.py) over the weights
    of the matching entries, for every counting case of the full list."""
    import test_gpu_replay_edges as T
    from xapiand_amd import _lib
    L = _lib.lib()
    n = 0
    for c in T.all_cases(False):
        if c.mode != T.REPLAY_COUNT:
            continue
        a = T.list_of(c)
        w = np.ascontiguousarray(a["weight"][(a["subqs"] & T.NOT) == 0])
        want = L.xgm_known_matching_docs(w.ctypes.data_as(C.POINTER(C.c_double)), len(w), c.k, c.cal)
        assert T.reference(c).known == want, (c.name, T.reference(c).known, want)
        n += 1
    assert n > 500


def test_reference_freezes_as_the_host_replay_does(built):
    """protomset(frozen_mode) = host_frozen_replay of tests/test_gpu_all.py (the loop the matcher hook ran on the host, pinned hook on == hook off against the
    compiled reference): page, count, max_weight and its subqs, on the thinned list's frozen cases — every branch, with and without a freeze."""
    import test_gpu_replay_edges as T
    from test_gpu_all import host_frozen_replay
    cases = T.frozen_cases(True) + [c for c in T.frozen_cases(False) if not c.tags[2]][:3]
    assert len(cases) >= 10
    for c in cases:
        a = T.list_of(c)
        conj = list(zip(a["docid"].tolist(), a["weight"].tolist(), a["subqs"].tolist()))
        matches = [h for h in conj if not h[2] & T.NOT]
        page, known, max_w, max_m = host_frozen_replay(matches, conj, c.k, c.cal)
        r = T.reference(c)
        assert r.page == tuple((d, T.bits(w), m) for d, w, m in page), c.name
        assert (r.known, r.max_w, r.max_m) == (known, max_w, max_m), (c.name, r.known, known)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not present")
def test_replay_edges_under_emulation(built):
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1", XGM_EMU_FAULT_TRACE="1")
    limit = 60 + 3 * 31                                              # the thinned list: 31 s measured (an event of the workgroup kernel costs about 20 ms emulated), with a factor of 3; pytest's start on top
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_replay_edges.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0 and "6 passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
