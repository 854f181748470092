"""ppe_classify_flow_host: a host-resident batch through the flow table, whatever the chunk size.

A warm-up batch and a batch of n packets over a shared flow population larger than the pool (so creators are revoked
with FLOW_NOMEM on both sides of chunk boundaries) go through the host call on one context, through ppe_classify_flow
from device buffers on a twin context, and through the oracle's sequential FlowHandlePacket as one batch each; all three
must agree in every per-packet output, the counters, the info counts and the dumped table.  Integer work: no
tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402
from test_gpu_flow import table  # noqa: E402
from test_gpu_portscan_host import GUARD, harr  # noqa: E402

DEV = torch.device("cuda:0")
NOW = 1_000_000
MAXB, CAP, FLOWS, WARM = 4096, 1500, 2500, 1000
OUTS = ("verdict", "flow_hash", "acl_hit", "tuple")
FILL = 0xFFFFFFF9
RULES = synth.make_rules(256, seed=21)


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    for x in e:
        x.commit(RULES, default_action=0)
    yield e
    for x in e:
        x.close()


def host_call(eng, hdr, lens, outs, ts=None, chunk=0, pinned=False, now=NOW, syn_check=1):
    """The raw host call with 64 guard entries behind every output; returns (rc, outputs by name, whole buffers)."""
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
            (np.uint32, FILL)
        arr, own = harr((sizes.get(k, n) + GUARD,), dtype, fill, pinned)
        keep.append((arr, own))
        bufs[k] = (arr, fill)
    g = lambda k: bufs[k][0].ctypes.data if k in bufs else None  # noqa: E731
    b = abi.Batch(h.ctypes.data, ln.ctypes.data, t.ctypes.data if t is not None else None, n, hdr.shape[1])
    r = abi.Result(g("verdict"), g("flow_hash"), g("acl_hit"), g("fw_idx"), g("drop_idx"), g("tile_cnt"), g("tuple"),
                   g("part8"), g("packed"))
    cfg = eng.cfg(0, syn_check, now)
    rc = eng.lib.ppe_classify_flow_host(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), int(chunk))
    res = {}
    for k, (arr, fill) in bufs.items():
        m = sizes.get(k, n)
        assert (arr[m:] == fill).all(), f"{k}: guard entries written"
        a = arr[:m].copy()
        res[k] = a.view(np.int32) if k == "acl_hit" else a
    if "tuple" in res:
        res["tuple"] = res["tuple"].reshape(n, 4)
    return rc, res, {k: v[0] for k, v in bufs.items()}


def device_call(eng, hdr, lens, ts, now):
    """One ppe_classify_flow of the batch from device buffers."""
    n = len(lens)
    out = {k: torch.full((n, 4) if k == "tuple" else (n,), -7, dtype=torch.int32, device=DEV) for k in OUTS}
    eng.classify_flow_torch(torch.from_numpy(np.ascontiguousarray(hdr)).to(DEV),
                            torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32)).to(DEV), out,
                            cfg=eng.cfg(0, 1, now), ts=torch.from_numpy(ts.view(np.int64)).to(DEV))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if k == "acl_hit" else v.cpu().numpy().view(np.uint32)) for k, v in out.items()}


def packets(n):
    """(warm-up batch, the n-packet batch, their timestamps) over one flow population."""
    w = synth.make_flow_packets(WARM, RULES, n_flows=FLOWS, seed=901, template_seed=900, kind="imix", stride=128,
                                malformed_frac=0.01)
    m = synth.make_flow_packets(n, RULES, n_flows=FLOWS, seed=902 + n, template_seed=900, kind="imix", stride=128,
                                malformed_frac=0.01)
    return (w["hdr"], w["len"], np.full(WARM, NOW, np.uint64)), (m["hdr"], m["len"], np.full(n, NOW + 1, np.uint64))


def state(eng):
    """The table, its counts and the counters.  (Not the tombstone count: a revoked claim leaves one per batch it was
    revoked in, so it depends on the chunking; no output does.)"""
    info = eng.flow_info()
    cnt = eng.counters()
    return (table(eng.flow_dump()), (info["live"], info["new_flow"], info["del_flow"]), [cnt[c] for c in abi.COUNTERS])


_ref = {}


def reference(engines, n):
    """The two batches through ppe_classify_flow on the twin (one batch each, device buffers) and through the oracle;
    computed once per n and checked against each other here."""
    if n not in _ref:
        twin = engines[1]
        warm, main = packets(n)
        twin.flow_create(CAP, max(MAXB, n))
        twin.clear_counters()
        o = pyoracle.Oracle(RULES, default_action=0)
        ft = pyoracle.OracleFlow(o, capacity=CAP)
        try:
            counters = np.zeros(32, np.uint64)
            for k, (hdr, lens, ts) in enumerate((warm, main)):
                got = device_call(twin, hdr, lens, ts, NOW + k)
                ref = ft.classify_batch(hdr, lens, ts=ts, cfg=o.cfg(0, 1, NOW + k))
                counters += ref["counters"]
                for name in OUTS:
                    assert np.array_equal(got[name], ref[name]), (name, k)
            tab, info, cnt = state(twin)
            st = ft.stats()
            assert tab == table(ft.dump()) and info == (st["live"], st["new_flow"], st["del_flow"])
            assert cnt == counters[:len(abi.COUNTERS)].tolist()
            _ref[n] = (warm, main, got, (tab, info, cnt))
        finally:
            twin.flow_destroy()
            ft.close()
    return _ref[n]


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("chunk", [64, 4096, 0])
@pytest.mark.parametrize("n", [1, 65, 4097, 20000])
def test_host_batch_is_one_cores_run(engines, n, chunk, pinned):
    warm, main, exp, exp_state = reference(engines, n)
    eng = engines[0]
    eng.flow_create(CAP, MAXB)
    eng.clear_counters()
    try:
        rc, _, _ = host_call(eng, *warm[:2], OUTS, ts=warm[2], chunk=chunk, pinned=pinned, now=NOW)
        assert rc == 0, (rc, eng.lib.ppe_last_error(eng.ctx))
        rc, got, _ = host_call(eng, *main[:2], OUTS, ts=main[2], chunk=chunk, pinned=pinned, now=NOW + 1)
        assert rc == 0, (rc, eng.lib.ppe_last_error(eng.ctx))
        for k in OUTS:
            assert np.array_equal(got[k], exp[k]), (k, np.flatnonzero((got[k] != exp[k]).reshape(n, -1).any(1))[:8])
        assert state(eng) == exp_state
        if n == 20000:  # the pool overflowed: creators were revoked in chunks past the first
            st = got["verdict"] & 0xFF
            assert (st[4096:] == abi.ST["FLOW_NOMEM"]).any() and exp_state[1][0] == CAP
    finally:
        eng.flow_destroy()


def test_python_wrapper_numpy_and_pinned(engines):
    """Engine.classify_flow_host with numpy arrays (staged) and with pinned torch tensors (read and written in place)."""
    warm, main, exp, exp_state = reference(engines, 4097)
    eng = engines[0]
    for pinned in (False, True):
        eng.flow_create(CAP, 8192)
        eng.clear_counters()
        try:
            for k, (hdr, lens, ts) in enumerate((warm, main)):
                if pinned:
                    pin = lambda a, d: torch.from_numpy(np.ascontiguousarray(a).view(d)).pin_memory()  # noqa: E731
                    out = {name: torch.full((len(lens), 4) if name == "tuple" else (len(lens),), -7,
                                            dtype=torch.int32).pin_memory() for name in OUTS}
                    eng.classify_flow_host(pin(hdr, np.uint8), pin(lens, np.int32), pin(ts, np.int64),
                                           cfg=eng.cfg(0, 1, NOW + k), out=out)
                    got = {name: (v.numpy() if name == "acl_hit" else v.numpy().view(np.uint32))
                           for name, v in out.items()}
                else:
                    got = eng.classify_flow_host(hdr, lens, ts, cfg=eng.cfg(0, 1, NOW + k), chunk=1000)
            for name in OUTS:
                assert np.array_equal(got[name], exp[name]), (name, pinned)
            assert state(eng) == exp_state
        finally:
            eng.flow_destroy()


def test_refusals_touch_nothing(engines):
    """Every refusal returns its code before anything is touched: the outputs keep the fill pattern and the table, its
    counts and the counters stay as they were."""
    warm, main, _, _ = reference(engines, 65)
    eng = engines[0]
    eng.flow_create(CAP, MAXB)
    eng.clear_counters()
    try:
        rc, _, _ = host_call(eng, *warm[:2], OUTS, ts=warm[2])
        assert rc == 0
        before = state(eng)

        def refused(code, outs=OUTS, pinned=False):
            rc, _, bufs = host_call(eng, *main[:2], outs, ts=main[2], pinned=pinned)
            assert rc == code, (rc, code, eng.lib.ppe_last_error(eng.ctx))
            for k, arr in bufs.items():
                fill = 0xEE if k == "part8" else 0xF9F9F9F9F9F9F9F9 if k == "packed" else FILL
                assert (arr == fill).all(), f"{k} written by a refused call"
            assert state(eng) == before

        for pinned in (False, True):
            # the layouts the host form does not take
            refused(abi.PPE_EINVAL, ("flow_hash", "acl_hit"), pinned)                      # no verdict
            for extra in ("fw_idx", "drop_idx", "tile_cnt", "part8", "packed"):
                refused(abi.PPE_EINVAL, ("verdict", extra), pinned)
            # the context states ppe_classify_flow refuses, and the monitors flow-attached
            eng.stream_tcp(1, 0, 0)
            refused(abi.PPE_ENOTSUP, pinned=pinned)
            eng.stream_tcp(0, 0, 0)
            ps = eng.portscan(capacity=64, max_batch=4096)
            refused(abi.PPE_ENOTSUP, pinned=pinned)
            ps.close()
            atk = eng.attack()
            refused(abi.PPE_ENOTSUP, pinned=pinned)
            atk.detach()
            atk.attach_flow()
            refused(abi.PPE_ENOTSUP, pinned=pinned)
            atk.close()
        # afterwards the call works and gives what the twin gave for the same two batches
        rc, got, _ = host_call(eng, *main[:2], OUTS, ts=main[2], now=NOW + 1)
        assert rc == 0
        _, _, exp, exp_state = reference(engines, 65)
        for k in OUTS:
            assert np.array_equal(got[k], exp[k]), k
        assert state(eng) == exp_state
    finally:
        eng.stream_tcp(0, 0, 0)
        eng.flow_destroy()


def test_no_table_small_table_and_broken_table(engines):
    _, main, _, _ = reference(engines, 65)
    eng = engines[0]
    rc, _, bufs = host_call(eng, *main[:2], OUTS, ts=main[2])
    assert rc == abi.PPE_EINVAL and all((a == FILL).all() for a in bufs.values())          # no table
    eng.flow_create(CAP, 63)
    try:
        rc, _, bufs = host_call(eng, *main[:2], OUTS, ts=main[2])
        assert rc == abi.PPE_EINVAL and all((a == FILL).all() for a in bufs.values())      # max_batch below a tile
        assert eng.flow_info()["live"] == 0
        eng.flow_create(CAP, MAXB)
        eng.lib.ppe_flow_debug_fail_post(1)
        rc, _, _ = host_call(eng, *main[:2], OUTS, ts=main[2])
        assert rc == -5                                                                    # PPE_EIO: the table broke
        rc, _, bufs = host_call(eng, *main[:2], OUTS, ts=main[2])
        assert rc == -5 and all((a == FILL).all() for a in bufs.values())                  # and stays unusable
    finally:
        eng.lib.ppe_flow_debug_fail_post(0)
        eng.flow_destroy()
