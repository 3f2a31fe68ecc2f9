"""CPU-only: the live set read natively from glass (xapiand_amd/csrc/xgm_glass.cc: xgm_glass_export_live — the docids of the doclen list, whatever
their length) on shards the REAL reference's driver builds (oracle/_ref/xapian_ref): the bits are the pattern the driver deletes by, they are
`doclen != 0` of the reference's own export (every document of these fixtures has a term with wdf > 0, so here the two agree), their number is the
version file's doccount, and the file attaches to the segment exported from the same shard — where, under the emulated kernels, xgm_filter_all hands
those bits back."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from xapiand_amd import _lib

pytestmark = pytest.mark.skipif(not H.have_xapian_ref(), reason="oracle/_ref/xapian_ref not built")

EMU = os.path.join(H.ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def misc_shard(tmp):
    """build_misc: 1 .. 3000 without the multiples of 5 (7 replaced: still there), then 40000, 70001, 3000000 and 3000001 .. 3002500."""
    db = os.path.join(tmp, "misc")
    H.xapian_ref("build_misc", db)
    live = np.zeros(3002501, dtype=bool)
    live[1:3001] = True
    live[5:3001:5] = False
    live[[40000, 70001, 3000000]] = True
    live[3000001:3002501] = True
    return db, live


def mutated_shard(tmp):
    """build 3000 documents, then append 1000 with mutate_from 1501: from the floor up every 7th docid deleted, every 11th replaced (still there)."""
    db = os.path.join(tmp, "mut")
    H.xapian_ref("build", db, H.CORPUS_SEED, 3000, 20000, 20, 60)
    out = json.loads(H.xapian_ref("append", db, H.CORPUS_SEED, 20001, 21000, 20000, 20, 60, 1501))
    assert out["last_before"] == 3000 and out["lastdocid"] == 4000
    live = np.ones(4001, dtype=bool)
    live[0] = False
    d = np.arange(1501, 3001)
    live[d[d % 7 == 0]] = False
    return db, live


def read_live_file(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"XGMLIV1\0"
    last, doccount, n_words, zero = np.frombuffer(raw, dtype="<u4", count=4, offset=8).tolist()
    assert n_words == (last + 32) // 32 and zero == 0 and len(raw) == 24 + 4 * n_words
    words = np.frombuffer(raw, dtype="<u4", offset=24)
    return last, doccount, words


CHILD = """
import sys
import numpy as np
from xapiand_amd import Database
db = Database(sys.argv[1])
db.attach_live_file(sys.argv[2])
f = db.filter_all()
np.array(f.words(), dtype=np.uint32).tofile(sys.argv[3])
print("n_docs", f.n_docs, db.get_doccount())
"""


@pytest.mark.parametrize("shard", [misc_shard, mutated_shard])
def test_exported_live_set(built, tmp_path, shard):
    db, live = shard(str(tmp_path))
    L = _lib.lib()
    path = str(tmp_path / "live.bin")
    _lib.check(L.xgm_glass_export_live(db.encode(), path.encode()))
    last, doccount, words = read_live_file(path)
    assert last == len(live) - 1
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert not bits[0] and not bits[last + 1:].any()
    assert (bits[:last + 1] == live).all(), np.nonzero(bits[:last + 1] != live)[0][:8]               # the pattern
    raw = str(tmp_path / "ref.raw")
    H.xapian_ref("export", db, raw)                                                                  # the reference's own export: "XGMRAW1", 4 u32, 5 u64, doclen[]
    doclen = np.fromfile(raw, dtype="<u4", count=last + 1, offset=64)
    assert ((doclen != 0) == bits[:last + 1]).all()
    dc, ld = C.c_uint32(), C.c_uint32()
    _lib.check(L.xgm_glass_info(db.encode(), None, C.byref(dc), C.byref(ld), None))
    assert int(bits.sum()) == dc.value == doccount == int(live.sum()) and ld.value == last
    assert dc.value != ld.value                                                                      # gaps: rule (a) would not answer for these shards
    assert L.xgm_glass_export_live(None, path.encode()) == _lib.XGM_E_INVALID and L.xgm_glass_export_live(db.encode(), None) == _lib.XGM_E_INVALID
    assert L.xgm_glass_export_live(str(tmp_path / "missing").encode(), path.encode()) == _lib.XGM_E_IO
    # the file and the segment of the same shard: on an index without a device the checks of the arguments come first, then XGM_E_NO_DEVICE
    seg = str(tmp_path / "s.seg")
    _lib.check(L.xgm_segment_build_from_glass(db.encode(), 0, seg.encode()))
    h = C.c_void_p()
    _lib.check(L.xgm_index_open(seg.encode(), _lib.XGM_DEVICE_NONE, _lib.UINT64_MAX, C.byref(h)))
    assert L.xgm_index_attach_live_file(h, path.encode()) == _lib.XGM_E_NO_DEVICE
    L.xgm_index_close(h)
    if not os.path.exists(CLANG):
        return
    # ... and on the emulated device it attaches, and xgm_filter_all returns those bits
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU])
    out = str(tmp_path / "words.bin")
    env = dict(os.environ, XGM_LIB_PATH=os.path.join(EMU, "libxgm_emu.so"), XGM_EMU_QUICK="1", XGM_EMU_GUARD="1",
               XGM_NO_DENSE="1", XGM_NO_FLAT="1")                       # (no accelerators: the live set reads none, and building them is the emulation's slowest part)
    r = subprocess.run([sys.executable, "-c", CHILD, seg, path, out], cwd=H.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "n_docs %d %d" % (doccount, doccount) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert (np.fromfile(out, dtype="<u4") == words).all()
