"""ppe_classify_host_ordered: a host-resident batch through the port-scan detector, whatever the chunk size.

A batch of 4,133 packets whose sources repeat across every chunk boundary, with scanners that first appear (and are
detected) in the second chunk of each chunk size, goes through the host call on one context and through one
ppe_classify from device buffers on a twin context; both are compared with the tests' serial model
(tests/portscan_model.py) and with each other: every output layout, both counter blocks, the info counts and the dumped
records.  Integer work: no tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import test_gpu_portscan as gp  # noqa: E402  (its rig: engine + model + oracle)
from portscan_model import DETECTED, HOLD, NOMEM, OK  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402

NOW, R, S0 = gp.NOW, gp.R, gp.S0
N, GUARD = 4133, 64
HOST_PACKED = ("packed", "part8")   # (the staged copies keep the packed words where the tuple would go)
LAYOUTS = (gp.SEP, gp.PART, gp.PART8, HOST_PACKED, gp.PLAIN)


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    yield e
    for x in e:
        x.close()


@pytest.fixture(autouse=True)
def clean_afterwards(request):
    yield
    if "engines" in request.fixturenames:
        for e in request.getfixturevalue("engines"):
            if getattr(e, "attack_attached", None) is not None:
                e.attack_attached.close()
            if getattr(e, "portscan_attached", None) is not None:
                e.portscan_attached.close()
            e.stream_tcp(0, 0, 0)


def harr(shape, dtype, fill, pinned):
    """A host array (pageable, or pinned and device-mapped through torch) filled with `fill`; returns (array, owner)."""
    if not pinned:
        return np.full(shape, fill, dtype), None
    t = torch.from_numpy(np.full(shape, fill, dtype).view({np.dtype(np.uint32): np.int32,
                                                            np.dtype(np.uint64): np.int64}.get(np.dtype(dtype), dtype)))
    t = t.pin_memory()
    return t.numpy().view(dtype), t


def host_call(eng, hdr, lens, outs, ts=None, chunk=0, pinned=False, syn_check=1, name="ppe_classify_host_ordered"):
    """The raw host call with 64 guard entries behind every output; returns (rc, outputs by name)."""
    n = len(lens)
    keep = []

    def inp(a, dtype):
        arr, own = harr(a.shape, dtype, 0, pinned)
        arr[...] = a
        keep.append((arr, own))
        return arr
    h, ln = inp(np.ascontiguousarray(hdr), np.uint8), inp(np.ascontiguousarray(lens, np.uint32), np.uint32)
    t = inp(np.ascontiguousarray(ts, np.uint64), np.uint64) if ts is not None else None
    sizes = {"tile_cnt": (n + 63) // 64, "tuple": 4 * n}
    bufs = {}
    for k in outs:
        dtype, fill = (np.uint8, 0xEE) if k == "part8" else (np.uint64, 0xF9F9F9F9F9F9F9F9) if k == "packed" else \
            (np.uint32, 0xFFFFFFF9)
        arr, own = harr((sizes.get(k, n) + GUARD,), dtype, fill, pinned)
        keep.append((arr, own))
        bufs[k] = (arr, fill)
    g = lambda k: bufs[k][0].ctypes.data if k in bufs else None  # noqa: E731
    fw, dr = (g("part_idx"), g("part_idx")) if "part_idx" in bufs else (g("fw_idx"), g("drop_idx"))
    b = abi.Batch(h.ctypes.data, ln.ctypes.data, t.ctypes.data if t is not None else None, n, hdr.shape[1])
    r = abi.Result(g("verdict"), g("flow_hash"), g("acl_hit"), fw, dr, g("tile_cnt"), g("tuple"), g("part8"), g("packed"))
    cfg = eng.cfg(0, syn_check, NOW)
    rc = getattr(eng.lib, name)(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), int(chunk))
    res = {}
    for k, (arr, fill) in bufs.items():
        m = sizes.get(k, n)
        assert (arr[m:] == fill).all(), f"{k}: guard entries written"
        a = arr[:m].copy()
        res[k] = a.view(np.int32) if k == "acl_hit" else a
    if "tuple" in res:
        res["tuple"] = res["tuple"].reshape(n, 4)
    if "packed" in res:
        res.update(abi.unpack(res["packed"]))
    if rc == 0 and "tile_cnt" in res and "fw_idx" in res:
        # the staging copies bring a tile's whole 64 list slots back: the slots behind a tile's count are not defined
        # through the host calls (ppe_classify leaves them untouched); give them the fill
        for t, tc in enumerate(res["tile_cnt"]):
            lo, hi = 64 * t, min(n, 64 * t + 64)
            res["fw_idx"][lo + (int(tc) & 0xFF):hi] = 0xFFFFFFF9
            res["drop_idx"][lo + ((int(tc) >> 8) & 0xFF):hi] = 0xFFFFFFF9
    return rc, res


class HostRig(gp.Rig):
    """tests/test_gpu_portscan.py's rig whose batches go through ppe_classify_host_ordered."""
    chunk, pinned = 0, False

    def classify(self, hdr, lens, outs, ts=None):
        rc, res = host_call(self.eng, hdr, lens, outs, ts, self.chunk, self.pinned, self.syn_check)
        assert rc == 0, (rc, self.eng.lib.ppe_last_error(self.eng.ctx))
        return res


_batch = {}


def crossing_batch(tcp):
    """(warm-up batch, the 4,133-packet batch): 40 sources against 24 records interleaved over the whole batch, and
    three scanners, known from the warm-up, whose packets start at 70, 130 and 1,100: inside the second chunk of 64,
    128 and 1,024 packets."""
    if tcp not in _batch:
        rng = np.random.default_rng(41)
        flags = 0x06 if tcp else None                       # SYN | RST: StreamTcp's RST-without-session verdict
        wsip = np.concatenate([(S0 + 200 + np.arange(3)).repeat(8), S0 + rng.integers(0, 20, 200)]).astype(np.uint32)
        wport = np.concatenate([np.tile(np.arange(1, 9), 3), rng.choice([22, 23, 80], 200)]).astype(np.uint32)
        sip = (S0 + rng.integers(0, 40, N)).astype(np.uint32)
        dport = rng.choice(np.array([0, 22, 22, 23, 80, 1000, 2000], np.uint32), N)
        for k, start in enumerate((70, 130, 1100)):
            idx = start + 5 * np.arange(30)
            sip[idx], dport[idx] = S0 + 200 + k, 3000 + np.arange(30)
        ts = np.full(N, NOW + 1, np.uint64)
        ts[3000:] = NOW + 700                               # past the hold: the held sources are released
        _batch[tcp] = (gp.frames(wsip, wport, tcp_flags=flags), gp.frames(sip, dport, tcp_flags=flags), ts)
    return _batch[tcp]


def twin_run(engines, chunk, pinned, outs, stream=None, max_batch=8192):
    """The warm-up and the crossing batch through the host call on engines[0] and through ppe_classify on engines[1]."""
    tcp = stream is not None
    (whdr, wlens), (hdr, lens), ts = crossing_batch(tcp)
    kw = dict(exception_freq=3, capacity=24, hold_seconds=600, stream=stream)
    host = HostRig(engines[0], gp.port_rules(), max_batch=max_batch, **kw)
    dev = gp.Rig(engines[1], gp.port_rules(), max_batch=8192, **kw)
    host.chunk, host.pinned = chunk, pinned
    try:
        for rig in (host, dev):
            rig.step(whdr, wlens)
            rig.clock(50_000 + R + 1, NOW + 1)
        ref = dev.reference(hdr, lens, ts)
        gd, exp = dev.step(hdr, lens, outs, ts, ref)            # one ppe_classify == the model
        gh, _ = host.step(hdr, lens, outs, ts, ref)             # the host call == the model
        for k in gh:
            assert np.array_equal(gh[k], gd[k][:len(gh[k])]), k     # (the device rig keeps part8's guard entries)
        assert engines[0].counters() == engines[1].counters()
        assert engines[0].stream_counters() == engines[1].stream_counters()
        assert {tuple(int(x) for x in e) for e in host.ps.dump()} == {tuple(int(x) for x in e) for e in dev.ps.dump()}
        res = exp["results"]
        for start in (70, 130, 1100):     # each scanner: a new port after the warm-up's window of 7 changes: detected
            assert res[start] == DETECTED and res[start + 5] == HOLD
        assert {OK, NOMEM, DETECTED, HOLD} <= set(res.tolist()) and (res[3000:] != HOLD).all()
        return host.ps.prepass_info(), exp
    finally:
        host.close()
        dev.close()


@pytest.mark.parametrize("chunk,outs", [(64, gp.SEP), (128, gp.PART), (1024, gp.PART8), (0, HOST_PACKED), (128, gp.PLAIN)],
                         ids=["64-sep", "128-part", "1024-part8", "0-packed", "128-plain"])
def test_pageable_chunks(engines, chunk, outs):
    """Pageable buffers: chunks of 64, 128 and 1,024 packets and the whole batch, each with another output layout."""
    info, _ = twin_run(engines, chunk, False, outs)
    last = N - (N - 1) // chunk * chunk if chunk else N         # the last chunk's packets: its pre-pass is the last one
    assert info == (1, 1) if last <= 2048 else info[0] == 0 and info[1] >= 10


def test_pinned_mapped_buffers_are_one_launch(engines):
    """Every buffer pinned and device-mapped: one pre-pass over all 4,133 packets (the staged launches), one launch."""
    info, _ = twin_run(engines, 64, True, gp.SEP)
    assert info[0] == 0 and info[1] >= 10


def test_copies_on_the_slots_streams(engines):
    """PPE_HOST_ORDERED_COPY=1 at context creation (the A/B switch): the copies stay on the staging slots' streams with an
    event each way; the same answer."""
    import os
    assert "PPE_HOST_ORDERED_COPY" not in os.environ
    os.environ["PPE_HOST_ORDERED_COPY"] = "1"
    try:
        eng = Engine(0)
    finally:
        del os.environ["PPE_HOST_ORDERED_COPY"]
    try:
        info, _ = twin_run((eng, engines[1]), 128, False, gp.SEP)
        assert info == (1, 1)
    finally:
        if getattr(eng, "portscan_attached", None) is not None:
            eng.portscan_attached.close()
        eng.close()


def test_stream_tcp_is_honoured(engines):
    """StreamTcp at the reference's defaults with TCP SYN|RST frames: RST_NO_SESSION for what the detector passes."""
    _, exp = twin_run(engines, 128, False, gp.PLAIN, stream=(1, 0, 0))
    st = exp["verdict"] & 0xFF
    assert (st == ST["STREAM_RST_NO_SESSION"]).sum() > 100 and (st == ST["PORTSCAN_DROP"]).sum() > 100


def test_chunk_is_clamped_to_max_batch(engines):
    """A table of max_batch 1,000: chunk 0 (the whole batch) and chunk 4,096 run as chunks of 960."""
    for chunk in (0, 4096):
        info, _ = twin_run(engines, chunk, False, gp.PLAIN, max_batch=1000)
        assert info == (1, 1)                                   # the last chunk: 4,133 - 4 * 960 = 293 packets
    info, _ = twin_run(engines, 64, True, gp.PLAIN, max_batch=1000)   # pinned, but larger than max_batch: chunks too
    assert info == (1, 1)


def test_without_a_table_it_is_classify_host(engines):
    """No table, a detached table and able = 0: equal to ppe_classify_host for every layout, pageable and pinned."""
    eng = engines[0]
    rules = synth.make_rules(256, seed=256)
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
    pk = synth.make_packets(N, rules, kind="imix", stride=128, malformed_frac=0.05)
    hdr, lens = pk["hdr"], pk["len"]

    def both(outs, pinned):
        eng.clear_counters()
        rc0, a = host_call(eng, hdr, lens, outs, chunk=128, pinned=pinned, name="ppe_classify_host")
        c0 = eng.counters()
        eng.clear_counters()
        rc1, b = host_call(eng, hdr, lens, outs, chunk=128, pinned=pinned)
        assert rc0 == rc1 == 0 and eng.counters() == c0
        for k in a:
            assert np.array_equal(a[k], b[k]), (outs, pinned, k)
        return b
    for outs in LAYOUTS:
        base = both(outs, False)
    both(gp.SEP, True)
    # packed with tuple needs device-mapped buffers, in both calls
    for name in ("ppe_classify_host", "ppe_classify_host_ordered"):
        assert host_call(eng, hdr, lens, ("packed", "tuple"), name=name)[0] == abi.PPE_EINVAL
    ps = eng.portscan(attach=False, exception_freq=0, capacity=8)
    ps.attach()
    ps.set(able=0)
    rc, got = host_call(eng, hdr, lens, gp.PLAIN, chunk=128)
    assert rc == 0 and all(np.array_equal(got[k], base[k]) for k in gp.PLAIN) and ps.info()["live"] == 0
    ps.close()


def test_refusals(engines):
    """Attack monitors attached: PPE_ENOTSUP and nothing written; ppe_classify_host with the table attached still
    returns PPE_ENOTSUP; afterwards the ordered call works."""
    eng = engines[0]
    (whdr, wlens), _, _ = crossing_batch(False)
    rig = HostRig(eng, gp.port_rules(), exception_freq=3, capacity=24)
    atk = eng.attack(None)
    try:
        eng.clear_counters()
        rc, res = host_call(eng, whdr, wlens, gp.SEP, chunk=64)
        assert rc == abi.PPE_ENOTSUP
        assert all((res[k].view(np.uint32) == 0xFFFFFFF9).all() for k in gp.SEP)
        assert rig.ps.info()["live"] == 0 and sum(eng.counters().values()) == 0
    finally:
        atk.close()
    rc, res = host_call(eng, whdr, wlens, ("verdict",), name="ppe_classify_host")
    assert rc == abi.PPE_ENOTSUP and (res["verdict"] == 0xFFFFFFF9).all() and rig.ps.info()["live"] == 0
    rig.step(whdr, wlens, outs=gp.SEP)
    rig.close()
