"""ppe_classify_flow_host with a port-scan table flow-attached: a host batch larger than one flow batch with the detector
inside runs as consecutive chunks of at most ppe_flow_portscan_max() packets, batch.ts taken per chunk, and the result is
one core's run of the whole batch whatever the chunk is.

4,133 generated packets (tests/flow_portscan_model.py: 8 sources and few tuples, so every source's detector chain and
many tuples cross every chunk boundary) behind a warm-up batch go through the host call in chunks of 64, 128, MAX and 0,
pageable and pinned; the outputs, counters and both tables must equal the model fed the whole batch, and a twin engine
fed consecutive device batches.  Integer work: no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import portscan_model as psm  # noqa: E402
import pyoracle  # noqa: E402
from ppe import Engine, abi  # noqa: E402
from test_gpu_flow import table  # noqa: E402
from test_gpu_flow_host import OUTS, host_call  # noqa: E402
from test_gpu_flow_portscan import PS_INFO  # noqa: E402

DEV = torch.device("cuda:0")
N, WARM = 4133, 300
PAR = dict(freq=2, hold=2, ps_capacity=8, flow_capacity=500, rate=1000)
CLOCKS = ((10_000, 1000), (11_500, 1001))  # (cycles, seconds) of the warm-up and of the batch: the window rolls
RULES = fpm.gen_rules()
DROP = abi.ACL_RULE_ACTION_DROP


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    for x in e:
        x.commit(RULES, default_action=DROP)
    yield e
    for x in e:
        x.close()


def packets():
    rng = np.random.default_rng(4133)
    out = []
    for n, (_, sec) in zip((WARM, N), CLOCKS):
        hdr, lens = fpm.gen_batch(rng, n)
        out.append((hdr, lens, (sec + rng.integers(0, 4, n)).astype(np.uint64)))
    return out


def setup(e):
    e.flow_create(PAR["flow_capacity"], 8192)
    e.clear_counters()
    return e.portscan(attach="flow", able=1, action=0, exception_freq=PAR["freq"], hold_seconds=PAR["hold"],
                      capacity=PAR["ps_capacity"], max_batch=8192, cycles_per_second=PAR["rate"])


def state(e, ps):
    """Both tables, their counts and the counters.  (Not the tombstone count: a creator-less claim leaves one per chunk
    it was made in, so it depends on the chunking; no output does.)"""
    info, cnt, pi = e.flow_info(), e.counters(), ps.info()
    return (table(e.flow_dump()), (info["live"], info["new_flow"], info["del_flow"]), [cnt[c] for c in abi.COUNTERS],
            {k: pi[k] for k in PS_INFO}, fpm.ps_records(ps.dump()))


_ref = {}


def reference(engines):
    """The model fed the two batches whole, and the twin engine fed consecutive device batches of MAX packets; computed
    once, checked against each other here, shared by every case."""
    if not _ref:
        twin = engines[1]
        mx = twin.flow_portscan_max()
        o = pyoracle.Oracle(RULES, default_action=DROP)
        m = fpm.FlowPortScanModel(o, PAR["flow_capacity"],
                                  psm.PortScanModel(1, 0, PAR["freq"], PAR["hold"], PAR["ps_capacity"], PAR["rate"]))
        ps = setup(twin)
        try:
            counters = np.zeros(32, np.uint64)
            for (hdr, lens, ts), (cyc, sec) in zip(packets(), CLOCKS):
                m.ps.clock(cyc, sec)
                ps.clock(cyc, sec)
                ref = m.classify_batch(hdr, lens, ts, o.cfg(0, 1, sec))
                counters += ref["counters"]
                got = {k: [] for k in OUTS}
                for lo in range(0, len(lens), mx):
                    n = len(lens[lo:lo + mx])
                    out = {k: torch.full((n, 4) if k == "tuple" else (n,), -7, dtype=torch.int32, device=DEV)
                           for k in OUTS}
                    twin.classify_flow_torch(torch.from_numpy(np.ascontiguousarray(hdr[lo:lo + mx])).to(DEV),
                                             torch.from_numpy(lens[lo:lo + mx].view(np.int32).copy()).to(DEV), out,
                                             cfg=twin.cfg(0, 1, sec),
                                             ts=torch.from_numpy(ts[lo:lo + mx].view(np.int64).copy()).to(DEV))
                    torch.cuda.synchronize()
                    assert twin.flow_launch_info() == (2, 1)
                    for k in OUTS:
                        a = out[k].cpu().numpy()
                        got[k].append(a if k == "acl_hit" else a.view(np.uint32))
                for k in OUTS:
                    assert np.array_equal(np.concatenate(got[k]), ref[k]), k
            st = m.stats()
            want = (m.table(), (st["live"], st["new_flow"], st["del_flow"]), counters[:len(abi.COUNTERS)].tolist(),
                    {k: m.ps.info()[k] for k in PS_INFO}, m.ps.records())
            assert state(twin, ps) == want
            assert all(m.events[k] > 0 for k in ("ok", "nomem", "detected", "hold", "creatorless_claim",
                                                 "found_of_held_source"))
            _ref["v"] = (ref, want)
        finally:
            ps.close()
            twin.flow_destroy()
    return _ref["v"]


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("chunk", [64, 128, "MAX", 0])
def test_host_batch_in_chunks(engines, chunk, pinned):
    ref, want = reference(engines)
    e = engines[0]
    ps = setup(e)
    try:
        c = e.flow_portscan_max() if chunk == "MAX" else chunk
        for k, ((hdr, lens, ts), (cyc, sec)) in enumerate(zip(packets(), CLOCKS)):
            ps.clock(cyc, sec)
            rc, got, _ = host_call(e, hdr, lens, OUTS, ts=ts, chunk=c, pinned=pinned, now=sec)
            assert rc == 0, e.lib.ppe_last_error(e.ctx)
            assert e.flow_launch_info() == (2, 1)
        for name in OUTS:
            assert np.array_equal(got[name], ref[name]), name
        assert state(e, ps) == want
    finally:
        ps.close()
        e.flow_destroy()


def test_small_pinned_batch_is_one_zero_copy_batch(engines):
    """n <= MAX with every buffer pinned: one flow batch read and written in place; the same answers as staged."""
    e = engines[0]
    res = []
    for pinned in (False, True):
        ps = setup(e)
        try:
            hdr, lens, ts = packets()[0]
            ps.clock(*CLOCKS[0])
            rc, got, _ = host_call(e, hdr, lens, OUTS, ts=ts, chunk=0, pinned=pinned, now=CLOCKS[0][1])
            assert rc == 0 and e.flow_launch_info() == (2, 1)
            res.append(([got[k].tobytes() for k in OUTS], state(e, ps)))
        finally:
            ps.close()
            e.flow_destroy()
    assert res[0] == res[1]


def test_refusals_touch_nothing(engines):
    e = engines[0]
    ps = setup(e)
    try:
        hdr, lens, ts = packets()[0]
        before = state(e, ps)
        rc, _, bufs = host_call(e, hdr, lens, OUTS + ("fw_idx",), ts=ts)   # lists: PPE_EINVAL, as without the detector
        assert rc == abi.PPE_EINVAL and all((b == b.flat[-1]).all() for b in bufs.values())
        e.stream_tcp(1, 0, 0)
        rc, _, bufs = host_call(e, hdr, lens, OUTS, ts=ts)
        e.stream_tcp(0, 0, 0)
        assert rc == abi.PPE_ENOTSUP and all((b == b.flat[-1]).all() for b in bufs.values())
        atk = e.attack(attach="flow")
        rc, _, bufs = host_call(e, hdr, lens, OUTS, ts=ts)
        atk.close()
        assert rc == abi.PPE_ENOTSUP and all((b == b.flat[-1]).all() for b in bufs.values())
        assert state(e, ps) == before
    finally:
        ps.close()
        e.flow_destroy()
