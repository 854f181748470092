"""ppe_defrag_host on the GPU: a batch in pageable host memory, run in chunks, against a twin table fed the same
chunks as device batches (ppe_defrag) and the oracle fed the whole batch at once.

Bar: status, datagram index, count, lengths, windows, whole frames and fragment-id lists bit-exact against the oracle
whatever the chunk, nothing written behind the datagram rows that exist or in the 64 guard entries, ppe_defrag_info
equal to the twin's and the oracle's, the same ids dropped by aging afterwards; the refusals write nothing."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from ppe import Defrag, Engine, abi, synth  # noqa: E402
from ppe.engine import PPEError  # noqa: E402

DEV = torch.device("cuda:0")
NOW = 1_000_000
GUARD = 64
ROOT = Path(__file__).resolve().parent.parent
CUT = int(re.search(r"#define PPE_DEFRAG_SMALL_CUTOFF (\d+)u",
                    (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()).group(1))
MAXB = 2048
PPE_EIO = -5
SMALL = min(CUT, 8)   # a batch the one-launch kernel takes


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def stream():
    """4,097 fragments (byte-aligned frames, so the host gather moves them) and the oracle's answer per prefix."""
    a, o, l = synth.make_fragment_stream(1400, seed=77, align=1)
    assert len(l) >= 4097
    ids = np.arange(len(l), dtype=np.uint64) * 7 + 5
    refs = {}
    for n in (1, 65, 4097):
        orc = pyoracle.OracleDefrag()
        try:
            refs[n] = (orc.batch(a, o[:n], l[:n], NOW, ids=ids[:n]), orc.stats(), orc.age(NOW + 10**6, 20))
        finally:
            orc.close()
    return a, o, l, ids, refs


def check(got, ref, n, stride, cm):
    nd = ref["n_dgram"]
    assert int(got["n_dgram"][0]) == nd and (got["n_dgram"][1:] == 0xA5A5A5A5).all()
    assert np.array_equal(got["status"][:n], ref["status"])
    assert np.array_equal(got["dgram_of"][:n], ref["dgram_of"])
    assert np.array_equal(got["dgram_len"][:nd], ref["dgram_len"][:nd])
    assert np.array_equal(got["dgram_frags"][:nd], ref["dgram_frags"][:nd])
    for j in range(nd):
        m = int(ref["dgram_len"][j])
        assert np.array_equal(got["dgram_pkt"][j, :m], ref["dgram_pkt"][j, :m]), f"datagram {j} bytes"
        w = np.zeros(stride, np.uint8)
        w[:min(m, stride)] = ref["dgram_pkt"][j, :min(m, stride)]
        assert np.array_equal(got["dgram_hdr"][j], w), f"datagram {j} window"
    # only the rows of datagrams that exist are written; the guard entries behind n stay
    assert (got["dgram_len"][nd:] == 0xA5A5A5A5).all() and (got["dgram_hdr"][nd:] == 0xA5).all()
    assert (got["dgram_pkt"][nd:] == 0xA5).all() and (got["dgram_frags"][nd:] == 0xA5A5A5A5A5A5A5A5).all()
    assert (got["status"][n:] == 0xA5A5A5A5).all() and (got["dgram_of"][n:] == 0xA5A5A5A5).all()


@pytest.mark.parametrize("chunk", [64, CUT, 0])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_host_batch_in_chunks(eng, stream, n, chunk):
    a, o, l, ids, refs = stream
    ref, stats, (aged, freed) = refs[n]
    g = Defrag(eng, max_batch=MAXB)
    twin = Defrag(eng, max_batch=MAXB)
    try:
        got = g.run_host(a, o[:n], l[:n], NOW, ids=ids[:n], chunk=chunk, guard=GUARD)
        check(got, ref, n, 128, g.info_["cache_max"])
        step = chunk or MAXB
        assert g.launch_info() == ((1, 1) if min(step, (n - 1) % step + 1) <= CUT else (0, 6))
        # the twin: the same chunks as device batches
        ta = torch.from_numpy(a).to(DEV)
        for b in range(0, n, step):
            m = min(step, n - b)
            out = twin.alloc_out(m, 128)
            twin.run_torch(ta, torch.from_numpy(o[b:b + m].view(np.int64)).to(DEV),
                           torch.from_numpy(l[b:b + m].view(np.int32)).to(DEV), out, NOW,
                           ids=torch.from_numpy(ids[b:b + m].view(np.int64)).to(DEV))
            st = out["status"].cpu().numpy().view(np.uint32)
            assert np.array_equal(st, got["status"][b:b + m])
        gi, ti = g.info(), twin.info()
        assert gi == ti
        for k, v in stats.items():
            assert gi[k] == v, (k, gi[k], v)
        di, df = g.age(NOW + 10**6, 20)
        assert df == freed and sorted(di.tolist()) == sorted(aged.tolist())
    finally:
        g.close()
        twin.close()


def test_without_ids_the_index_in_the_whole_batch(eng, stream):
    a, o, l, _, _ = stream
    n = 300
    orc = pyoracle.OracleDefrag()
    g = Defrag(eng, max_batch=MAXB)
    try:
        ref = orc.batch(a, o[:n], l[:n], NOW)
        got = g.run_host(a, o[:n], l[:n], NOW, chunk=64, hdr_stride=64, guard=GUARD)
        check(got, ref, n, 64, g.info_["cache_max"])
    finally:
        g.close()
        orc.close()


def raw_call(g, a, o, l, n, drop=(), stride=128):
    """ppe_defrag_host on filled outputs with the pointers named in drop NULL: (return code, outputs untouched)."""
    arr = dict(status=np.full(n, 0xA5A5A5A5, np.uint32), dgram_of=np.full(n, 0xA5A5A5A5, np.uint32),
               dgram_hdr=np.full((n, 128), 0xA5, np.uint8), dgram_len=np.full(n, 0xA5A5A5A5, np.uint32),
               n_dgram=np.full(1, 0xA5A5A5A5, np.uint32))
    src = dict(pkt=a, off=np.ascontiguousarray(o[:n]), len=np.ascontiguousarray(l[:n]))
    p = lambda k: None if k in drop else arr[k].ctypes.data
    q = lambda k: None if k in drop else src[k].ctypes.data
    b = abi.FragBatch(q("pkt"), q("off"), q("len"), None, n, 0, NOW)
    out = abi.DefragOut(p("status"), p("dgram_of"), p("dgram_hdr"), p("dgram_len"), None, None, p("n_dgram"), stride, 0)
    rc = g.lib.ppe_defrag_host(g.h, C.byref(b), C.byref(out), 0)
    return rc, all((v == (0xA5 if v.dtype == np.uint8 else 0xA5A5A5A5)).all() for v in arr.values())


def test_refusals_write_nothing(eng, stream):
    a, o, l, _, _ = stream
    n = 65
    g = Defrag(eng, max_batch=MAXB)
    try:
        for drop in (("pkt",), ("off",), ("len",), ("status",), ("dgram_hdr",), ("dgram_len",)):
            assert raw_call(g, a, o, l, n, drop) == (abi.PPE_EINVAL, True), drop
        assert raw_call(g, a, o, l, n, stride=96) == (abi.PPE_EINVAL, True)
        assert g.lib.ppe_defrag_host(g.h, None, None, 0) == abi.PPE_EINVAL
        assert g.info()["running"] == 0 and g.launch_info() == (0, 0)   # nothing ran
        assert raw_call(g, a, o, l, n) == (0, False)                    # the same call, complete: runs
        assert raw_call(g, a, o, l, n, ("dgram_of", "n_dgram"))[0] == 0  # the optional ones absent
    finally:
        g.close()


def test_pending_lookback_error_is_eio_and_writes_nothing(eng, stream, monkeypatch):
    """A six-launch batch whose admission look-back failed (the PPE_DF_LOOK_FAIL hook): the next ppe_defrag_host
    returns PPE_EIO once, before it writes anything, and the table goes on."""
    a, o, l, _, _ = stream
    monkeypatch.setenv("PPE_DF_LOOK_FAIL", "1")
    g = Defrag(eng, max_batch=MAXB)
    monkeypatch.delenv("PPE_DF_LOOK_FAIL")
    try:
        assert raw_call(g, a, o, l, 1024)[0] == 0             # 4 admission workgroups: workgroup 1's look-back fails
        assert g.launch_info() == (0, 6)
        assert raw_call(g, a, o, l, SMALL) == (PPE_EIO, True)
        with pytest.raises(PPEError):
            g.info()                                          # the device counter of failed look-backs (then cleared)
        assert raw_call(g, a, o, l, SMALL) == (0, False)
        assert g.launch_info() == (1, 1)
    finally:
        g.close()


def test_a_small_chunk_waits_for_the_armed_hook(eng, stream, monkeypatch):
    """While the hook is armed (until the table's first batch) a small chunk stays on the six launches."""
    a, o, l, _, _ = stream
    monkeypatch.setenv("PPE_DF_LOOK_FAIL", "1")
    g = Defrag(eng, max_batch=MAXB)
    monkeypatch.delenv("PPE_DF_LOOK_FAIL")
    try:
        assert raw_call(g, a, o, l, SMALL)[0] == 0 and g.launch_info() == (0, 6)
        assert raw_call(g, a, o, l, SMALL)[0] == 0 and g.launch_info() == (1, 1)
    finally:
        g.close()
