"""Host batches with ppe_flow_stream_portscan on: ppe_classify_flow_host as launch kind 7 per chunk with its slice of `ts`,
ppe_classify_flow_host_ports as kind 8 per chunk with its slices of `ports` and `ts`; a 2,500-packet batch in chunks of
64 / 128 / MAX / 0, pageable and pinned, against the model fed the whole batch as one; the pinned zero-copy form at
n <= MAX; the refusals.  The flow path, the detector and the sessions are sequential and between two ticks no verdict
reads an accumulator, so the chunk size changes nothing (only the table's tombstone count may differ)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import test_flow_stream_portscan_model as tsp  # noqa: E402
from ppe import PPEError  # noqa: E402
from test_gpu_flow_stream_portscan import KINDS, MAX, engines, gen_rig, pool  # noqa: E402,F401

COLS = ("verdict", "flow_hash", "acl_hit", "tuple")
N = 2500


def batch(n, seed=51):
    hdr, lens, ports = pool(seed, n)
    return hdr, lens, ports, np.sort(1000 + np.arange(n) * 3 // n).astype(np.uint64)


def host_call(rig, hdr, lens, ports, ts, chunk=0, out=None):
    e = rig.eng
    if rig.kind == 8:
        return e.classify_flow_host_ports(hdr, lens, ports, ts, cfg=e.cfg(0, 1, 1000), chunk=chunk, outputs=COLS, out=out)
    return e.classify_flow_host(hdr, lens, ts, cfg=e.cfg(0, 1, 1000), chunk=chunk, outputs=COLS, out=out)


def expect(rig, hdr, lens, ports, ts):
    exp, reasons = rig.mod.classify_batch(hdr, lens, ports, ts, rig.mod.o.cfg(0, 1, 1000))
    rig.counters += exp["counters"].astype(np.int64)
    return exp, reasons


@KINDS
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("chunk", [64, 128, "MAX", 0])
def test_host_batch_in_chunks(engines, MAX, kind, chunk, pinned):
    chunk = MAX if chunk == "MAX" else chunk
    _, par = tsp.generated()
    # (a pool of 32 flows: this batch holds 63 tuples that would create one, so FLOW_NOMEM occurs in mid-chunk)
    rig = gen_rig(engines[0], kind, dict(par, flow_capacity=32), max_batch=1 << 14)
    try:
        hdr, lens, ports, ts = batch(N)
        rig.clock(10_000, 1000)
        if pinned:
            th, tl = torch.from_numpy(hdr.copy()).pin_memory(), torch.from_numpy(lens.copy().view(np.int32)).pin_memory()
            tt = torch.from_numpy(ts.copy().view(np.int64)).pin_memory()
            tp = torch.from_numpy(ports.copy()).pin_memory()
            out = {k: torch.full((4 * N,) if k == "tuple" else (N,), -7, dtype=torch.int32).pin_memory() for k in COLS}
            host_call(rig, th, tl, tp, tt, chunk, out)
            got = {k: out[k].numpy().view(np.int32 if k == "acl_hit" else np.uint32) for k in COLS}
            got["tuple"] = got["tuple"].reshape(-1, 4)
        else:
            got = host_call(rig, hdr, lens, ports, ts, chunk)
        exp, reasons = expect(rig, hdr, lens, ports, ts)
        for k in COLS:
            assert np.array_equal(got[k], exp[k]), (k, chunk)
        st = set((exp["verdict"] & 0xFF).tolist())
        assert reasons.any() and {tsp.P24, tsp.FNOMEM, tsp.AFW} <= st
        assert rig.eng.flow_launch_info() == (kind, 1)
        rig.same(f"host chunk {chunk}")
    finally:
        rig.close()


@KINDS
def test_a_small_pinned_batch_takes_the_zero_copy_form(engines, MAX, kind):
    _, par = tsp.generated()
    rig = gen_rig(engines[0], kind, par)
    try:
        hdr, lens, ports, ts = batch(MAX, seed=52)
        rig.clock(10_000, 1000)
        th, tl = torch.from_numpy(hdr.copy()).pin_memory(), torch.from_numpy(lens.copy().view(np.int32)).pin_memory()
        tt, tp = torch.from_numpy(ts.copy().view(np.int64)).pin_memory(), torch.from_numpy(ports.copy()).pin_memory()
        out = {k: torch.full((4 * MAX,) if k == "tuple" else (MAX,), -7, dtype=torch.int32).pin_memory() for k in COLS}
        host_call(rig, th, tl, tp, tt, 0, out)
        exp, _ = expect(rig, hdr, lens, ports, ts)
        assert np.array_equal(out["verdict"].numpy().view(np.uint32), exp["verdict"])
        assert np.array_equal(out["tuple"].numpy().view(np.uint32).reshape(-1, 4), exp["tuple"])
        assert rig.eng.flow_launch_info() == (kind, 1)
        rig.same("zero copy")
    finally:
        rig.close()


def test_the_refusals(engines):
    eng = engines[0]
    _, par = tsp.generated()
    rig = gen_rig(eng, 8, par)
    try:
        hdr, lens, ports, ts = batch(200, seed=53)
        rig.clock(10_000, 1000)
        cfg = eng.cfg(0, 1, 1000)
        with pytest.raises(PPEError, match="-95"):  # ppe_classify_flow_host keeps refusing monitors flow-attached
            eng.classify_flow_host(hdr, lens, ts, cfg=cfg, chunk=64)
        eng.flow_stream_portscan(0)
        with pytest.raises(PPEError, match="-95"):  # the switch off: the refusal it always was
            eng.classify_flow_host_ports(hdr, lens, ports, ts, cfg=cfg, chunk=64)
        eng.flow_stream_portscan(1)
        eng.flow_combine(0)
        with pytest.raises(PPEError, match="-95"):
            eng.classify_flow_host_ports(hdr, lens, ports, ts, cfg=cfg, chunk=64)
        eng.flow_combine(1)
        with pytest.raises(PPEError, match="-22"):  # a header stride under 144 B
            eng.classify_flow_host_ports(np.ascontiguousarray(hdr[:, :128]), lens, ports, ts, cfg=cfg, chunk=64)
        eng.stream_tcp(track=1, reasm=1)
        with pytest.raises(PPEError, match="-95"):
            eng.classify_flow_host_ports(hdr, lens, ports, ts, cfg=cfg, chunk=64)
        eng.stream_tcp(track=1, reasm=0)
        rig.same("after the refusals")
        got = eng.classify_flow_host_ports(hdr, lens, ports, ts, cfg=cfg, chunk=64, outputs=COLS)
        exp, _ = expect(rig, hdr, lens, ports, ts)
        for k in COLS:
            assert np.array_equal(got[k], exp[k]), k
        rig.same("after the refusals, a batch")
    finally:
        rig.close()
