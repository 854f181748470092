"""ppe_classify_flow_host_ports with the monitors flow-attached, sessions attached and ppe_flow_stream_monitors on: a
3,000-packet host batch with a port byte per packet in chunks of 64 / 1,024 / 0 against the model fed the whole batch
and against a twin engine fed device batches; the pinned zero-copy form at n <= ppe_flow_stream_max(); ports NULL.
Sessions are sequential and between two ticks no verdict reads an accumulator, so the chunk size changes nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

from test_gpu_flow import table  # noqa: E402
from test_gpu_flow_stream_attack import MAX, NOW, PD, TD, Rig, engines, generated  # noqa: E402,F401

COLS = ("verdict", "flow_hash", "acl_hit", "tuple")
N = 3000


def warm(rig, hdr, lens, ports):
    """An interval of traffic and a tick, so that the floods' rates are above their thresholds in the batch under test."""
    rig.step(hdr[N:N + 200], lens[N:N + 200], ports[N:N + 200], what="warm")
    rig.tick(NOW + 1)


@pytest.mark.parametrize("chunk", [64, 1024, 0])
def test_host_batch_in_chunks(engines, generated, MAX, chunk):
    hdr, lens, ports = generated
    host, twin = (Rig(e, pd=PD, td=TD, max_batch=1 << 14) for e in engines)
    try:
        for r in (host, twin):
            warm(r, hdr, lens, ports)
        got = host.eng.classify_flow_host_ports(hdr[:N], lens[:N], ports[:N], cfg=host.eng.cfg(0, 1, NOW + 1), chunk=chunk,
                                                outputs=COLS)
        exp, reasons = host.expect(hdr[:N], lens[:N], ports[:N], NOW + 1)
        for k in COLS:
            assert np.array_equal(got[k], exp[k]), (k, chunk)
        st = set((exp["verdict"] & 0xFF).tolist())
        assert reasons.any() and {26, 28} <= st and host.eng.flow_launch_info() == (6, 1)
        host.same(f"host chunk {chunk}")
        for pos in range(0, N, MAX):  # the twin: the same packets as device batches
            sl = slice(pos, min(pos + MAX, N))
            twin.step(hdr[sl], lens[sl], ports[sl], now=NOW + 1, what=f"twin {pos}")
        assert table(host.eng.flow_dump()) == table(twin.eng.flow_dump())
        assert host.atk.info() == twin.atk.info()
        assert host.eng.counters() == twin.eng.counters()
        host.tick(NOW + 2)
    finally:
        host.close()
        twin.close()


def test_a_small_pinned_batch_takes_the_zero_copy_form_and_ports_null(engines, generated, MAX):
    hdr, lens, ports = generated
    rig = Rig(engines[0], pd=PD, td=TD)
    try:
        warm(rig, hdr, lens, ports)
        th, tl = torch.from_numpy(hdr[:MAX].copy()).pin_memory(), torch.from_numpy(lens[:MAX].copy().view(np.int32)).pin_memory()
        tp = torch.from_numpy(ports[:MAX].copy()).pin_memory()
        out = {k: torch.full((4 * MAX,) if k == "tuple" else (MAX,), -7, dtype=torch.int32).pin_memory() for k in COLS}
        rig.eng.classify_flow_host_ports(th, tl, tp, cfg=rig.eng.cfg(0, 1, NOW + 1), out=out)
        exp, _ = rig.expect(hdr[:MAX], lens[:MAX], ports[:MAX], NOW + 1)
        assert np.array_equal(out["verdict"].numpy().view(np.uint32), exp["verdict"])
        assert np.array_equal(out["tuple"].numpy().view(np.uint32).reshape(-1, 4), exp["tuple"])
        assert rig.eng.flow_launch_info() == (6, 1)
        rig.same("zero copy")
        sl = slice(MAX, MAX + 500)  # ports NULL: port 0 for every packet
        got = rig.eng.classify_flow_host_ports(hdr[sl], lens[sl], None, cfg=rig.eng.cfg(0, 1, NOW + 1), chunk=128, outputs=COLS)
        exp, _ = rig.expect(hdr[sl], lens[sl], None, NOW + 1)
        for k in COLS:
            assert np.array_equal(got[k], exp[k]), k
        rig.same("ports NULL")
    finally:
        rig.close()
