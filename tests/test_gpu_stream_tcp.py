"""StreamTcp's first-packet verdict on the stateless classify path (ppe_stream_tcp_set) on the GPU, bit-exact against
the oracle's result rewritten by the tests' model (tests/stream_model.py): verdict word, flow hash, ACL hit, tuple,
the FW / DROP lists and tile counts, the partition list, its compact form, the packed words, and both counter blocks.

The batch is synth.make_tcp_flag_sweep: every value of the low six TCP flag bits x a zero / non-zero ack field x
{plain, one VLAN tag, ihl = 6 (the TCP header behind an IPv4 option, read by the kernel's slow path)}, UDP and
malformed packets between them, 64 k + 37 packets.  Integer work: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
import decode_corpus as dc  # noqa: E402
import stream_model as sm  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402

NOW = 1_700_000_000
DEV = torch.device("cuda:0")
SEP = ("verdict", "flow_hash", "acl_hit", "fw_idx", "drop_idx", "tile_cnt", "tuple")  # the general kernel
PART = ("verdict", "flow_hash", "acl_hit", "part_idx")                                 # the throughput-layout kernel
PART8 = ("verdict", "flow_hash", "acl_hit", "part8")
PACKED = ("packed", "part8")
OFF, REF_DEFAULT, MIDSTREAM, ONESIDE = (0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1)
STREAM_ST = (ST["STREAM_RST_NO_SESSION"], ST["STREAM_FIN_NO_SESSION"], ST["STREAM_MIDSTREAM_ONESIDE_OFF"],
             ST["STREAM_MIDSTREAM_OFF"])


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def tracking_off_afterwards(request):
    yield
    if "eng" in request.fixturenames:
        request.getfixturevalue("eng").stream_tcp(0, 0, 0)


def ruleset(name):
    """(rules, default action): FW-all (no rule, default FW), or make_rules sets with default FW, whose DROP rules
    leave some TCP packets ACL-dropped (256: whole image in LDS; 4096: a split image with cut lists)."""
    if name == "fwall":
        return np.zeros(0, abi.RULE_DTYPE), abi.ACL_RULE_ACTION_FW
    return synth.make_rules(int(name), seed=int(name)), abi.ACL_RULE_ACTION_FW


_cache = {}


def sweep(rules_name, stride, repeat=1):
    """The sweep batch over a rule set, computed once."""
    key = ("pk", rules_name, stride, repeat)
    if key not in _cache:
        _cache[key] = synth.make_tcp_flag_sweep(ruleset(rules_name)[0], stride=stride, repeat=repeat)
    return _cache[key]


def oracle_ref(rules_name, stride, repeat, syn_check):
    """The oracle's answer (tracking off) for the sweep, computed once per case and left unchanged."""
    key = ("ref", rules_name, stride, repeat, syn_check)
    if key not in _cache:
        rules, dflt = ruleset(rules_name)
        pk = sweep(rules_name, stride, repeat)
        o = pyoracle.Oracle(rules, default_action=dflt)
        ref = o.classify_batch(pk["hdr"], pk["len"], cfg=o.cfg(0, syn_check, NOW), nthreads=4)
        assert (ref["reach"] <= 128).all()  # a 128-B window holds every header of the sweep: nothing to mask there
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def gpu_classify(eng, hdr, lens, outs, syn_check=1):
    n = len(lens)
    th = torch.from_numpy(np.ascontiguousarray(hdr)).to(DEV)
    tl = torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32)).to(DEV)
    shapes = {"tile_cnt": ((n + 63) // 64,), "tuple": (n, 4)}
    out = {k: torch.full(shapes.get(k, (n,)), -7, dtype=torch.int32, device=DEV) for k in outs
           if k not in ("part8", "packed")}
    if "part8" in outs:  # (64 guard bytes past n: the compact list must not write beyond its n entries)
        out["part8"] = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    if "packed" in outs:
        out["packed"] = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    eng.classify_torch(th, tl, out, cfg=eng.cfg(0, syn_check, NOW))
    torch.cuda.synchronize()
    res = {}
    for k, v in out.items():
        a = v.cpu().numpy()
        res[k] = a if k in ("acl_hit", "part8") else a.view(np.uint64) if k == "packed" else a.view(np.uint32)
    return res


def same(name, got, want, keep=None):
    if keep is not None:
        got, want = got[keep], want[keep]
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError(f"{name}: {len(bad)} mismatches, first {bad[:5].tolist()}: gpu={got[bad[:3]].tolist()} "
                             f"model={want[bad[:3]].tolist()}")


def check_against_model(eng, pk, ref, cfg, stride, outs, syn_check=1, counters=True):
    """One classify of the sweep with `outs`; everything it wrote against the model.  At stride 64 the packets whose
    headers reach past the window (the oracle's reach > 64; malformed ones only) are WINDOW_PUNTs and excluded from
    the per-packet comparison; at stride 128 nothing is excluded."""
    n = len(pk["len"])
    eng.clear_counters()
    eng.clear_stream_counters()
    got = gpu_classify(eng, pk["hdr"], pk["len"], outs, syn_check)
    if "packed" in got:
        got.update(abi.unpack(got["packed"]))
    near = ref["reach"] <= stride
    assert stride == 64 or near.all()
    assert ((got["verdict"][~near] & 0xFF) == ST["WINDOW_PUNT"]).all()
    r = dict(ref)
    if not near.all():  # the model sees what the kernel saw for the punted packets: not tracked
        r["verdict"] = np.where(near, ref["verdict"], got["verdict"])
    exp = sm.expected(r, pk["hdr"], dict(zip(("track", "midstream", "async_oneside"), cfg)))
    for k in ("verdict", "flow_hash", "acl_hit") + (("tuple",) if "tuple" in got else ()):
        same(k, got[k], exp[k], near)
    if "packed" in got:
        same("packed", got["packed"], sm.packed(exp["verdict"], exp["flow_hash"], exp["acl_hit"]), near)
    # compaction sees the new DROP action: the lists the (checked) verdicts imply
    want = sm.lists(np.where(near, exp["verdict"], got["verdict"]))
    for k in ("fw_idx", "drop_idx", "tile_cnt", "part_idx"):
        if k in got:
            same(k, got[k], want[k])
    if "part8" in got:
        same("part8", got["part8"][:n], want["part8"])
        assert (got["part8"][n:] == 0xEE).all()
    assert eng.stream_counters() == exp["stream"]
    if counters and near.all():
        assert eng.counters() == exp["counters"]
    return got, exp


CASES = [(c, s) for c in (OFF, REF_DEFAULT, MIDSTREAM, ONESIDE) for s in (1, 0) if not (c == MIDSTREAM and s == 0)]


@pytest.mark.parametrize("rules_name", ["fwall", "256"])
@pytest.mark.parametrize("cfg,syn_check", CASES, ids=[f"t{c[0]}m{c[1]}a{c[2]}-syn{s}" for c, s in CASES])
def test_config_states(eng, rules_name, cfg, syn_check):
    """Every setting x syn_check (minus the unsupported pair) over the sweep at stride 128, all four output layouts:
    bit-exact against the model, both counter blocks exact."""
    rules, dflt = ruleset(rules_name)
    eng.commit(rules, default_action=dflt)
    assert eng.stream_tcp(*cfg) == dict(track=cfg[0], midstream=cfg[1], async_oneside=cfg[2], reasm=cfg[0])
    pk, ref = sweep(rules_name, 128), oracle_ref(rules_name, 128, 1, syn_check)
    for outs in (SEP, PART, PART8, PACKED):
        got, exp = check_against_model(eng, pk, ref, cfg, 128, outs, syn_check)
    st = got["verdict"] & 0xFF
    hit = {s: int((st == s).sum()) for s in STREAM_ST}
    if cfg == OFF:
        assert not any(hit.values())
    else:  # the sweep reaches every branch the setting leaves open
        assert hit[ST["STREAM_RST_NO_SESSION"]] > 0 and hit[ST["STREAM_FIN_NO_SESSION"]] > 0
        assert (hit[ST["STREAM_MIDSTREAM_ONESIDE_OFF"]] > 0) == (cfg == REF_DEFAULT)
        assert (hit[ST["STREAM_MIDSTREAM_OFF"]] > 0) == (syn_check == 0)
        assert exp["stream"]["pkt_broken_ack"] > 0 and exp["stream"]["syn_count"] > 0
    if rules_name == "256":
        assert int((st == ST["ACL_DROP"]).sum()) > 0  # some TCP never reaches StreamTcp


# every launch tuning of tests/test_gpu_parity.py's kernel-variant test (a copy: that file stays as it is)
TUNINGS = [dict(lds_image=0), dict(block=512), dict(block=1024), dict(block=256), dict(pipeline=1),
           dict(pipeline=4), dict(pipeline=1, block=256), dict(pipeline=1, block=512), dict(pipeline=1, lds_image=0),
           dict(pipeline=4, lds_image=0), dict(pipeline=4, block=1024), dict(blocks_per_cu=16), dict(blocks_per_cu=1),
           dict(pipeline=3), dict(pipeline=3, lds_image=0), dict(pipeline=5), dict(pipeline=5, block=1024),
           dict(pipeline=5, lds_image=0), dict(pipeline=5, block=256)]


@pytest.mark.parametrize("tune", TUNINGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("stride", [64, 128])
def test_kernel_variants(eng, tune, stride):
    """The reference's default setting under every kernel variant: image in global memory / LDS / split, the four
    tile fetch modes (single tile, hoisted, multi-tile rounds, cut lists), workgroup and grid sizes, the general and
    the throughput-layout kernels; 256 rules (whole image in LDS) and 4096 (split image, cut lists); the sweep four
    times over (2,149 packets) so the multi-tile rounds have whole rounds to run."""
    for rules_name in ("256", "4096"):
        rules, dflt = ruleset(rules_name)
        eng.commit(rules, default_action=dflt)
        eng.stream_tcp(*REF_DEFAULT)
        pk, ref = sweep(rules_name, stride, 4), oracle_ref(rules_name, stride, 4, 1)
        old = eng.tuning()
        try:
            eng.tuning(**tune)
            for outs in (SEP, PART, PACKED):
                got, _ = check_against_model(eng, pk, ref, REF_DEFAULT, stride, outs)
        finally:
            eng.tuning(**old)
        assert int(np.isin(got["verdict"] & 0xFF, STREAM_ST).sum()) > 500


def test_off_means_off(eng):
    """Tracking set, then cleared: the next launch equals the oracle unmodified and the stream counters stand still
    (the setting travels with each launch: no sync, nothing sticky)."""
    rules, dflt = ruleset("256")
    eng.commit(rules, default_action=dflt)
    pk, ref = sweep("256", 128), oracle_ref("256", 128, 1, 1)
    eng.stream_tcp(*REF_DEFAULT)
    check_against_model(eng, pk, ref, REF_DEFAULT, 128, SEP)
    before = eng.stream_counters()
    assert before["rst_but_no_session"] > 0
    eng.stream_tcp(0, 0, 0)
    eng.clear_counters()
    got = gpu_classify(eng, pk["hdr"], pk["len"], SEP)
    for k in ("verdict", "flow_hash", "acl_hit", "tuple"):
        same(k, got[k], ref[k])
    assert eng.stream_counters() == before
    assert eng.counters() == dict(zip(abi.COUNTERS, (int(x) for x in ref["counters"])))
    # ppe_counters_clear keeps its meaning: it leaves the stream counters alone, and the other way round
    eng.clear_counters()
    assert eng.stream_counters() == before
    eng.clear_stream_counters()
    assert not any(eng.stream_counters().values()) and not any(eng.counters().values())


def test_batches_ring_path(eng):
    """ppe_classify_batches over 34 sweep-sized batches (more than the kernel arguments hold: the device descriptor
    ring, one persistent launch): each batch bit-exact against the model, the counters the sum."""
    rules, dflt = ruleset("256")
    eng.commit(rules, default_action=dflt)
    eng.tuning(batches_per_launch=0)
    eng.stream_tcp(*REF_DEFAULT)
    pk, ref = sweep("256", 128), oracle_ref("256", 128, 1, 1)
    exp = sm.expected(ref, pk["hdr"], dict(track=1))
    want = sm.lists(exp["verdict"])
    n, nb = len(pk["len"]), 34
    keep = []
    for j in range(nb):
        m = n - j  # ragged: every batch ends in a different partial tile
        th = torch.from_numpy(pk["hdr"][:m].copy()).to(DEV)
        tl = torch.from_numpy(pk["len"][:m].view(np.int32).copy()).to(DEV)
        out = {k: torch.full((m,), -7, dtype=torch.int32, device=DEV) for k in ("verdict", "flow_hash", "acl_hit", "part")}
        b = abi.Batch(th.data_ptr(), tl.data_ptr(), None, m, 128)
        r = abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(),
                       out["part"].data_ptr(), out["part"].data_ptr(), None, None)
        keep.append((b, r, th, tl, out, m))
    ins = (abi.Batch * nb)(*(k[0] for k in keep))
    outs = (abi.Result * nb)(*(k[1] for k in keep))
    cfg = eng.cfg(0, 1, NOW)
    s = torch.cuda.current_stream(DEV)
    eng.clear_counters()
    eng.clear_stream_counters()
    assert eng.lib.ppe_classify_batches(eng.ctx, ins, outs, nb, C.byref(cfg), C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    total = dict.fromkeys(abi.STREAM_COUNTERS, 0)
    for _, _, _, _, out, m in keep:
        for k in ("verdict", "flow_hash"):
            same(k, out[k].cpu().numpy().view(np.uint32), exp[k][:m])
        same("acl_hit", out["acl_hit"].cpu().numpy(), exp["acl_hit"][:m])
        part = sm.lists(exp["verdict"][:m])["part_idx"] if m != n else want["part_idx"]
        same("part_idx", out["part"].cpu().numpy().view(np.uint32), part)
        e = sm.expected({k: v[:m] if k != "counters" else v for k, v in ref.items()}, pk["hdr"][:m], dict(track=1))
        for k, v in e["stream"].items():
            total[k] += v
    assert eng.stream_counters() == total
    assert eng.counters()["pkts"] == sum(k[5] for k in keep)


@pytest.mark.parametrize("memory", ["pinned", "pinned-staged", "pageable"])
def test_host_path(eng, monkeypatch, memory):
    """ppe_classify_host: pinned buffers (zero-copy), pinned with the staged copies, and pageable memory in chunks
    (internal streams, their own counter slot sets): bit-exact against the model, both counter blocks exact."""
    if memory == "pinned-staged":
        monkeypatch.setenv("PPE_HOST_ZEROCOPY", "0")
    rules, dflt = ruleset("256")
    eng.commit(rules, default_action=dflt)
    eng.stream_tcp(*REF_DEFAULT)
    pk, ref = sweep("256", 128), oracle_ref("256", 128, 1, 1)
    exp = sm.expected(ref, pk["hdr"], dict(track=1))
    n = len(pk["len"])
    pin = (lambda t: t.pin_memory()) if memory != "pageable" else (lambda t: t)
    ph = pin(torch.from_numpy(pk["hdr"].copy()))
    pl = pin(torch.from_numpy(pk["len"].view(np.int32).copy()))
    out = {k: pin(torch.full((n,), -7, dtype=torch.int32)) for k in ("verdict", "flow_hash", "acl_hit", "part")}
    b = abi.Batch(ph.data_ptr(), pl.data_ptr(), None, n, 128)
    r = abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(),
                   out["part"].data_ptr(), out["part"].data_ptr(), None, None)
    cfg = eng.cfg(0, 1, NOW)
    eng.clear_counters()
    eng.clear_stream_counters()
    assert eng.lib.ppe_classify_host(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), 128) == 0  # 128-packet chunks
    same("verdict", out["verdict"].numpy().view(np.uint32), exp["verdict"])
    same("flow_hash", out["flow_hash"].numpy().view(np.uint32), exp["flow_hash"])
    same("acl_hit", out["acl_hit"].numpy(), exp["acl_hit"])
    same("part_idx", out["part"].numpy().view(np.uint32), sm.lists(exp["verdict"])["part_idx"])
    assert eng.stream_counters() == exp["stream"]
    assert eng.counters() == exp["counters"]


def test_decode_shim_reads_the_settings():
    """The drop-in layer: with stream_tcp_track_enable = 1 a SYN|ACK mbuf reaches the drop hook and a SYN mbuf the
    forward hook; with 0 (the library's start value) both forward.  Stream drops are not logged (flow.c:316-319)."""
    from pktbuild import tcp_packet
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = abi.load()
    hook = C.CFUNCTYPE(None, C.POINTER(abi.Mbuf))
    assert lib.DP_Acl_Rule_Init() == 0
    lib.ppe_rule_list_free()
    assert lib.ppe_rule_list_init() == 0
    rule = np.zeros(1, abi.RULE_DTYPE)  # one rule the test's packets do not match (a commit needs a changed list)
    rule["sip"], rule["sip_mask"], rule["dip_mask"], rule["protocol_start"], rule["protocol_end"] = 0x01020304, 32, 0, 17, 17
    rule["sport_end"] = rule["dport_end"] = 65535
    rule["action"] = abi.ACL_RULE_ACTION_DROP
    rid = C.c_uint32()
    assert lib.Rule_add(rule.ctypes.data, C.byref(rid)) == 0
    dflt = C.c_uint32.in_dll(lib, "dp_acl_action_default")
    track = C.c_uint32.in_dll(lib, "stream_tcp_track_enable")
    old = dflt.value
    dflt.value = abi.ACL_RULE_ACTION_FW
    logged = []
    alert = hook(lambda m: logged.append(1))
    try:
        assert lib.DP_Acl_Rule_Commit() == 0
        lib.reg_fw_alert.argtypes = [hook]
        lib.reg_fw_alert(alert)
        frames = [tcp_packet(flags=0x12, payload=b"\0" * 10), tcp_packet(flags=0x02, payload=b"\0" * 10)]
        bufs = [C.create_string_buffer(f, len(f)) for f in frames]
        for on, want in ((1, {"fw": [1], "drop": [0]}), (0, {"fw": [0, 1], "drop": []}), (1, {"fw": [1], "drop": [0]})):
            track.value = on
            mb = (abi.Mbuf * 2)()
            for i in range(2):
                mb[i].pkt_ptr = C.cast(bufs[i], C.c_void_p).value
                mb[i].pkt_totallen = len(frames[i])
            base, sz = C.addressof(mb), C.sizeof(abi.Mbuf)
            got = {"fw": [], "drop": [], "punt": []}
            hooks = tuple(hook(lambda m, k=k: got[k].append((C.addressof(m.contents) - base) // sz))
                          for k in ("fw", "drop", "punt"))
            lib.ppe_set_output_hooks.argtypes = [hook, hook, hook]
            lib.ppe_set_output_hooks(*hooks)
            lib.Decode_Set_Burst(1000)
            for i in range(2):
                lib.Decode(C.byref(mb[i]))
            assert lib.Decode_Flush() == 2
            lib.ppe_set_output_hooks(hook(), hook(), hook())
            assert (sorted(got["fw"]), got["drop"], got["punt"]) == (want["fw"], want["drop"], []), on
            st0 = mb[0].ppe_verdict & 0xFF
            assert st0 == (ST["STREAM_MIDSTREAM_ONESIDE_OFF"] if on else ST["ACL_FW"])
            assert mb[0].ppe_acl_hit == -1 and (mb[0].ppe_verdict >> 16) & abi.F_ACL
            assert mb[1].ppe_verdict & 0xFF == ST["ACL_FW"]
        assert not logged
    finally:
        track.value = 0
        dflt.value = old
        lib.reg_fw_alert(hook())
        lib.ppe_rule_list_free()


def test_errors(eng):
    """PPE_EINVAL for a word above 1; PPE_ENOTSUP for track && midstream && !syn_check on each stateless call and
    for ppe_classify_flow with tracking on, which leaves the flow table usable: after resetting the setting it
    still matches the oracle's flow table on a 4096-packet batch."""
    lib = eng.lib
    eng.stream_tcp(0, 0, 0)
    for bad in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2), (1, 0, 0, 0xFFFFFFFF)):
        c = abi.StreamTcpCfg(*bad)
        assert lib.ppe_stream_tcp_set(eng.ctx, C.byref(c)) == abi.PPE_EINVAL
    got = abi.StreamTcpCfg(9, 9, 9, 9)
    assert lib.ppe_stream_tcp_get(eng.ctx, C.byref(got)) == 0 and got.as_dict() == dict(
        track=0, midstream=0, async_oneside=0, reasm=0)  # a refused setting changes nothing
    assert lib.ppe_stream_tcp_get(eng.ctx, None) == abi.PPE_EINVAL
    assert lib.ppe_stream_tcp_set(eng.ctx, None) == 0  # NULL: the reference's defaults
    assert lib.ppe_stream_tcp_get(eng.ctx, C.byref(got)) == 0 and got.as_dict() == dict(
        track=1, midstream=0, async_oneside=0, reasm=1)

    rules, dflt = ruleset("256")
    eng.commit(rules, default_action=dflt)
    pk = synth.make_flow_packets(4096, rules, n_flows=600, seed=21, syn_frac=0.6)
    th = torch.from_numpy(pk["hdr"]).to(DEV)
    tl = torch.from_numpy(pk["len"].view(np.int32)).to(DEV)
    out = {k: torch.full((4096,), -7, dtype=torch.int32, device=DEV) for k in ("verdict", "flow_hash", "acl_hit")}
    b = abi.Batch(th.data_ptr(), tl.data_ptr(), None, 4096, 64)
    r = abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(), None, None,
                   None, None)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    nosyn, syn = eng.cfg(0, 0, NOW), eng.cfg(0, 1, NOW)
    eng.stream_tcp(1, 1, 0)
    assert lib.ppe_classify(eng.ctx, C.byref(b), C.byref(r), C.byref(nosyn), s) == abi.PPE_ENOTSUP
    assert lib.ppe_classify_batches(eng.ctx, C.byref(b), C.byref(r), 1, C.byref(nosyn), s) == abi.PPE_ENOTSUP
    hh, hl = pk["hdr"][:256].copy(), pk["len"][:256].copy()
    hv = np.full(256, 0xFFFFFFF9, np.uint32)
    hb = abi.Batch(hh.ctypes.data, hl.ctypes.data, None, 256, 64)
    hr = abi.Result(hv.ctypes.data, None, None, None, None, None, None)
    assert lib.ppe_classify_host(eng.ctx, C.byref(hb), C.byref(hr), C.byref(nosyn), 0) == abi.PPE_ENOTSUP
    torch.cuda.synchronize()
    assert (out["verdict"].cpu().numpy() == -7).all() and (hv == 0xFFFFFFF9).all()  # nothing ran
    assert lib.ppe_classify(eng.ctx, C.byref(b), C.byref(r), C.byref(syn), s) == 0  # with syn_check it is supported

    eng.flow_create(10_000, 4096)
    o = pyoracle.Oracle(rules, default_action=dflt)
    ft = pyoracle.OracleFlow(o, capacity=10_000)
    try:
        eng.stream_tcp(*REF_DEFAULT)
        assert lib.ppe_classify_flow(eng.ctx, C.byref(b), C.byref(r), C.byref(syn), s) == abi.PPE_ENOTSUP
        with pytest.raises(PPEError, match="-95"):
            eng.classify_flow_torch(th, tl, out, cfg=syn)
        from ppe.dist import DeviceSteerOps, steered_classify_flow
        with pytest.raises(PPEError, match="-95"):  # before any collective: no process group is needed to see it
            steered_classify_flow(DeviceSteerOps(eng), None, th, tl, syn, 1, 0)
        eng.stream_tcp(0, 0, 0)
        assert eng.flow_info()["live"] == 0  # the refused calls touched nothing
        eng.classify_flow_torch(th, tl, out, cfg=syn)
        torch.cuda.synchronize()
        ref = ft.classify_batch(pk["hdr"], pk["len"], cfg=o.cfg(0, 1, NOW))
        same("verdict", out["verdict"].cpu().numpy().view(np.uint32), ref["verdict"])
        same("flow_hash", out["flow_hash"].cpu().numpy().view(np.uint32), ref["flow_hash"])
        same("acl_hit", out["acl_hit"].cpu().numpy(), ref["acl_hit"])
        assert eng.flow_info()["live"] == ft.stats()["live"] > 0
    finally:
        eng.flow_destroy()
        ft.close()


def corpus_case(rules_name, stride, syn_check):
    """The decode edge corpus (tests/decode_corpus.py) through a stride-wide window and the oracle's answer for it
    (tracking off), computed once per case and left unchanged."""
    key = ("corpus", rules_name, stride, syn_check)
    if key not in _cache:
        rules, dflt = ruleset(rules_name)
        if ("corpus", rules_name) not in _cache:
            _cache[("corpus", rules_name)] = dc.corpus(rules)
        hdr, lens, _ = _cache[("corpus", rules_name)]
        pk = dict(hdr=np.ascontiguousarray(hdr[:, :stride]), len=lens)
        o = pyoracle.Oracle(rules, default_action=dflt)
        ref = o.classify_batch(pk["hdr"], pk["len"], cfg=o.cfg(0, syn_check, NOW))
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = (pk, ref)
    return _cache[key]


@pytest.mark.parametrize("tune", [dict(), dict(pipeline=3), dict(pipeline=5)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()) or "default")
@pytest.mark.parametrize("cfg", [REF_DEFAULT, ONESIDE], ids=["default", "oneside"])
@pytest.mark.parametrize("stride", [128, 64])
def test_decode_edge_corpus(eng, tune, cfg, stride):
    """TCP flag bytes and th_ack behind every IPv4 header length 5 to 15 and both tag types (the slow path's reads of
    them), next to every malformed neighbour of such a frame: the decode edge corpus with tracking on.  At stride 64
    the frames behind long options are WINDOW_PUNTs, excluded as for the sweep."""
    for rules_name in ("256", "4096"):
        rules, dflt = ruleset(rules_name)
        eng.commit(rules, default_action=dflt)
        eng.stream_tcp(*cfg)
        old = eng.tuning()
        try:
            eng.tuning(**tune)
            for syn_check in (1, 0):
                pk, ref = corpus_case(rules_name, stride, syn_check)
                for outs in (SEP, PART):
                    got, exp = check_against_model(eng, pk, ref, cfg, stride, outs, syn_check)
                assert exp["stream"]["syn_count"] > 0 and exp["stream"]["syn_ack_count"] > 0
                if syn_check == 0:
                    assert exp["stream"]["rst_but_no_session"] > 0 and exp["stream"]["fin_but_no_session"] > 0
                    assert exp["stream"]["midstream_disable"] > 0 and exp["stream"]["pkt_broken_ack"] > 0
        finally:
            eng.tuning(**old)

