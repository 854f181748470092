"""ppe_classify_flow_host with the TCP session machine attached: the generated conversations (a few thousand packets)
as one host batch in chunks of 64 / 128 / MAX / 0, pageable and pinned, against the model fed the whole batch and
against a twin engine fed device batches.  The flow path and the sessions are exactly sequential, so the chunk size
changes nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import stream_session_model as m  # noqa: E402
from ppe import abi  # noqa: E402
from test_gpu_flow_stream import NOW, Rig, engines, generated, MAX  # noqa: E402,F401
from test_gpu_flow import table  # noqa: E402

COLS = ("verdict", "flow_hash", "acl_hit", "tuple")


def pinned(hdr, lens):
    th, tl = torch.from_numpy(hdr.copy()).pin_memory(), torch.from_numpy(lens.copy().view(np.int32)).pin_memory()
    n = len(lens)
    out = {k: torch.full((4 * n,) if k == "tuple" else (n,), -7, dtype=torch.int32).pin_memory() for k in COLS}
    return th, tl, out


@pytest.mark.parametrize("chunk", [64, 128, "MAX", 0])
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
def test_host_batch_in_chunks(engines, generated, MAX, chunk, pin):
    seq, hdr, lens = generated
    chunk = MAX if chunk == "MAX" else chunk
    n = len(lens)
    host, twin = Rig(engines[0], max_batch=1 << 14), Rig(engines[1], max_batch=1 << 14)
    try:
        cfg = host.eng.cfg(0, 1, NOW)
        if pin:  # (n > MAX: the staged path, from pinned buffers)
            th, tl, out = pinned(hdr, lens)
            host.eng.classify_flow_host(th, tl, cfg=cfg, chunk=chunk, out=out)
            got = {k: out[k].numpy().view(np.int32 if k == "acl_hit" else np.uint32) for k in COLS}
            got["tuple"] = got["tuple"].reshape(n, 4)
        else:
            got = host.eng.classify_flow_host(hdr, lens, cfg=cfg, chunk=chunk, outputs=COLS)
        exp, reasons = host.expect(hdr, lens, NOW)
        for k in COLS:
            assert np.array_equal(got[k], exp[k]), (k, chunk, pin)
        assert reasons.any() and host.eng.flow_launch_info() == (5, 1)
        host.same(f"host chunk {chunk}")
        # the twin: the same packets as device batches of MAX
        for pos in range(0, n, MAX):
            twin.step(hdr[pos:pos + MAX], lens[pos:pos + MAX], what=f"twin {pos}")
        assert table(host.eng.flow_dump()) == table(twin.eng.flow_dump())
        assert host.eng.stream_track_counters() == twin.eng.stream_track_counters()
        assert host.eng.counters() == twin.eng.counters()
        key = lambda e: (e.sip, e.dip, e.sport, e.dport)  # noqa: E731
        a, b = (sorted(((key(e), e.state, e.flags, e.client.astuple(), e.server.astuple())
                        for e in r.eng.flow_stream_dump())) for r in (host, twin))
        assert a == b and len(a) > 100
    finally:
        host.close()
        twin.close()


def test_a_small_pinned_batch_takes_the_zero_copy_form(engines, generated, MAX):
    """n <= MAX with every buffer pinned and device-mapped: the kernel reads and writes the host buffers, one batch."""
    seq, hdr, lens = generated
    rig = Rig(engines[0])
    try:
        th, tl, out = pinned(hdr[:MAX], lens[:MAX])
        rig.eng.classify_flow_host(th, tl, cfg=rig.eng.cfg(0, 1, NOW), out=out)
        exp, _ = rig.expect(hdr[:MAX], lens[:MAX], NOW)
        assert np.array_equal(out["verdict"].numpy().view(np.uint32), exp["verdict"])
        assert np.array_equal(out["tuple"].numpy().view(np.uint32).reshape(-1, 4), exp["tuple"])
        rig.same("zero copy")
    finally:
        rig.close()
