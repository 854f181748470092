"""The reassembly edge corpus (tests/defrag_corpus.py) keeps its promises, checked on the CPU against the oracle's
sequential Defrag: every hand-derived status list is what the oracle answers, alone and in every arrangement; every
status value and the teardrop bit occur; the chain inserts, datagram lengths, segment ends and source phases the GPU
tests rely on are really there; and the reassembly's parse agrees with the decoder's on what a fragment is."""
import numpy as np
import pytest

import pyoracle
from pktbuild import arena as plain_arena, ip_checksum_ok, ip_frag

import defrag_corpus as dfc

NOW = 1_000_000


@pytest.fixture(scope="module")
def cs():
    return dfc.cases()


def fields(fr, n):
    """(l2, ihl*4, frag_len, protocol) of an accepted fragment frame of wire length n."""
    l2 = 18 if bytes(fr[12:14]) in (b"\x81\x00", b"\x91\x00") else 14
    ihl4 = (fr[l2] & 15) * 4
    return l2, ihl4, (n & 0xFFFF) - l2 - ihl4, fr[l2 + 9]


@pytest.fixture(scope="module")
def alone(cs):
    """Every case run alone in one batch (ids = the frame's index): name -> the oracle's result."""
    out = {}
    for c in cs:
        d = pyoracle.OracleDefrag(**dfc.oracle_cfg(c.cfg))
        a, o, l = dfc.arena(c.frames)
        out[c.name] = d.batch(a, o, l, NOW)
        d.close()
    return out


def run(cs, batches, cfg, align=4, fcb_max=None, want=None):
    """A whole sequence through one oracle table: the statuses by gid, and the statuses wanted."""
    d = pyoracle.OracleDefrag(**dfc.oracle_cfg(cfg, fcb_max))
    a, bts = dfc.layout(cs, batches, align, want)
    n = sum(len(b[1]) for b in bts)
    got, exp = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for k, (off, lens, gid, w) in enumerate(bts):
        r = d.batch(a, off, lens, NOW + k, ids=gid)
        got[gid.astype(np.int64)] = r["status"]
        exp[gid.astype(np.int64)] = w
        if len(bts) > 1:
            assert d.age(NOW + k, dfc.NEVER)[0].size == 0
    s = d.stats()
    d.close()
    return got, exp, s


def test_corpus_is_deterministic_named_and_keyed(cs):
    again = dfc.cases()
    assert [c.name for c in cs] == [c.name for c in again]
    assert all(a.frames == b.frames and a.want == b.want and a.cols == b.cols for a, b in zip(cs, again))
    assert len({c.name for c in cs}) == len(cs) and len({c.key for c in cs}) == len(cs)
    assert {c.cfg for c in cs} == set(dfc.CONFIGS) and len(dfc.CONFIGS) == 3
    assert all(v["fcb_max"] <= 1024 for v in dfc.CONFIGS.values())
    assert sum(len(c.frames) for c in cs) < 600 and max(max(c.cols) for c in cs) + 1 <= 17
    for c in cs:
        assert len(c.frames) == len(c.want) == len(c.cols) > 0
        assert len(c.frames) == 1 or c.family != "A"
        for fr, n in c.frames if c.family != "A" else ():   # the case's key is in every frame of a chain
            ip = fr[fields(fr, n)[0]:]
            assert tuple(int.from_bytes(ip[x:y], "big") for x, y in ((12, 16), (16, 20), (4, 6))) == c.key
    # the builder's new keyword arguments change nothing for its earlier callers
    old = ip_frag(17, 1, 2, 3, 16, True, b"abcdefgh", ihl=6, vlan_tag=True, pad=2)
    assert old == ip_frag(17, 1, 2, 3, 16, True, b"abcdefgh", ihl=6, vlan_tag=True, pad=2, etype=0x8100, inner=0x0800,
                          ver=4, ip_len=32, offw=0x2002)
    assert old[12:14] == b"\x81\x00" and old[16:18] == b"\x08\x00" and old[18] == 0x46 and len(old) == 18 + 24 + 8 + 2


def test_arena_fills_the_gaps_and_hits_every_phase(cs):
    fr = [f for c in cs for f in c.frames]
    for align in (1, 4):
        a, off, lens = dfc.arena(fr, align)
        covered = np.zeros(len(a), bool)
        for (b, n), o in zip(fr, off):
            assert bytes(a[int(o):int(o) + len(b)]) == b
            assert a[int(o) + len(b)] == dfc.FILL                      # at least one filler byte behind every frame
            covered[int(o):int(o) + len(b)] = True
        assert (a[~covered] == dfc.FILL).all() and (~covered[-dfc.TAIL:]).all()
        assert np.array_equal(lens, [n for _, n in fr])
        assert set((off & 3).tolist()) == ({0, 1, 2, 3} if align == 1 else {0})
    # the arena of pktbuild (zero filler) is not the corpus's
    assert plain_arena([fr[0][0]])[0][-1] == 0


def test_every_case_alone_gives_its_hand_derived_statuses(cs, alone):
    bad = [(c.name, alone[c.name]["status"].tolist(), c.want) for c in cs if alone[c.name]["status"].tolist() != c.want]
    assert not bad, bad[:5]
    # every rejected parse row has an accepted neighbour of the same tagging
    for t in dfc.TAGS:
        w = {c.want[0] for c in cs if c.name.startswith(f"A/{t}/")}
        assert w == {dfc.NOT_FRAG, dfc.CACHED, dfc.HW2SW_ERR}


@pytest.mark.parametrize("cfg", list(dfc.CONFIGS))
def test_every_arrangement_gives_the_same_statuses(cs, cfg):
    sub = dfc.of_config(cs, cfg)
    seen = []
    for align in (4, 1):
        for name, batches in dfc.arrangements(sub):
            got, exp, _ = run(sub, batches, cfg, align)
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (name, align, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
            seen.append(name)
    assert seen == ["together", "interleaved", "columns"] * 2
    cols = dict(dfc.arrangements(sub))["columns"]
    assert len(cols) == max(len(c.frames) for c in sub) and sorted(x for b in cols for x in b) == \
        sorted(dict(dfc.arrangements(sub))["together"][0])


def test_fcb_full_group_fails_exactly_the_last_creators(cs):
    g, fcb_max, want = dfc.fcb_full_group(cs)
    assert fcb_max == len(g) - 2 >= 4 and all(len(c.frames) >= 2 for c in g[-2:])
    assert any(dfc.HW2SW_ERR in c.want for c in g[:-2] + g[-2:])
    for name, batches in dfc.arrangements(g):
        got, exp, s = run(g, batches, "default", fcb_max=fcb_max, want=want)
        assert np.array_equal(got, exp), name
        nfail = sum(len(c.frames) for c in g[-2:])
        assert (got == dfc.FCB_FULL).sum() == nfail and (got[-nfail:] == dfc.FCB_FULL).all()
        assert s["running"] == fcb_max == s["new_fcb"] and s["st_fcb_full"] == nfail


def test_every_status_and_the_teardrop_bit_occur(cs, alone):
    seen = set()
    for c in cs:
        seen |= set(alone[c.name]["status"].tolist())
    g, fcb_max, want = dfc.fcb_full_group(cs)
    seen |= set(run(g, dict(dfc.arrangements(g))["together"], "default", fcb_max=fcb_max, want=want)[0].tolist())
    assert {s & 0xFF for s in seen} == set(range(9))
    assert dfc.DEFRAG_ERR | dfc.TEAR in seen and dfc.DEFRAG_ERR in seen


def test_inserts_at_the_ends_of_a_full_nibble_list(cs, alone):
    """With 15 fragments chained, the 16th goes to chain position 0 in one case and strictly inside in another: the
    datagram's fragment list (chain order) against the arrival order (ids = arrival index)."""
    r0, r14 = alone["B/cm16_insert_at_0"], alone["B/cm16_insert_at_14"]
    assert r0["n_dgram"] == r14["n_dgram"] == 1
    assert r0["dgram_frags"][0].tolist() == [15] + list(range(15))
    assert r14["dgram_frags"][0].tolist() == list(range(14)) + [15, 14]
    assert alone["B/cm16_append_17"]["status"].tolist() == [dfc.CACHED] * 16 + [dfc.CACHE_FULL]
    assert alone["B/reverse_completes"]["dgram_frags"][0, :4].tolist() == [2, 1, 3, 0]


def test_datagrams_lengths_segments_checksums_and_payload_order(cs, alone):
    lens, starts, ends, head_lens, srcs, n_plain, n_icmp = set(), set(), set(), set(), set(), 0, 0
    a1, bts = dfc.layout(cs, dict(dfc.arrangements(cs))["together"], align=1)
    off1 = bts[0][0]
    base = np.cumsum([0] + [len(c.frames) for c in cs])
    for ci, c in enumerate(cs):
        r = alone[c.name]
        if r["n_dgram"] == 0:
            assert c.payload is None
            continue
        assert r["n_dgram"] == 1 and c.want.count(dfc.REASM) == 1
        n = int(r["dgram_len"][0])
        lens.add(min(n // 64, 2))
        chain = [int(x) for x in r["dgram_frags"][0] if x != 2**64 - 1]
        f = [fields(*c.frames[k]) for k in chain]
        l2, ihl4, _, proto = f[0]
        head_lens.add(min(c.frames[chain[0]][1] // 64, 2))
        dg = bytes(r["dgram_pkt"][0, :min(n, dfc.CONFIGS[c.cfg]["reasm_buf_bytes"])])
        assert n == c.frames[chain[0]][1] + sum(x[2] for x in f[1:])
        if proto == 1:   # the head frame with ip_off cleared, then zeros
            n_icmp += 1
            hf = c.frames[chain[0]][0]
            assert c.payload is None and dg[:l2 + 6] == hf[:l2 + 6] and dg[l2 + 6:l2 + 8] == b"\0\0"
            assert dg[l2 + 8:len(hf)] == hf[l2 + 8:] and dg[len(hf):] == bytes(n - len(hf)) and n > len(hf)
            continue
        n_plain += 1
        assert c.payload is not None, c.name
        assert ip_checksum_ok(dg[l2:l2 + ihl4]), c.name
        assert int.from_bytes(dg[l2 + 2:l2 + 4], "big") == ihl4 + len(c.payload) and dg[l2 + 6:l2 + 8] == b"\0\0"
        assert dg[l2 + ihl4:] == c.payload, c.name
        assert dg[:l2] == c.frames[chain[0]][0][:l2]
        dst = c.frames[chain[0]][1]
        for k, x in zip(chain[1:], f[1:]):
            starts.add(dst & 3)
            dst += x[2]
            ends.add(dst & 3)
            srcs.add((int(off1[base[ci] + k]) + c.frames[k][1] - x[2]) & 3)
    assert lens == {0, 1, 2} and head_lens == {0, 1, 2}          # < 64, 64..127, >= 128: both window paths
    assert n_plain >= 20 and n_icmp >= 4
    # offsets are multiples of 8 and a completed chain tiles [0, total): a later segment starts at l2 + ihl*4 + 8k
    assert starts == {2}
    assert ends == {0, 1, 2, 3} and srcs == {0, 1, 2, 3}


def test_the_two_oracles_agree_on_what_a_fragment_is():
    """The decode corpus's frames through OracleDefrag: NOT_FRAG exactly where the decoder's oracle does not report
    status FRAG."""
    from ppe import abi, synth
    import decode_corpus as dc
    rules = synth.make_rules(256, seed=256)
    hdr, lens, meta = dc.corpus(rules)
    o = pyoracle.Oracle(rules, default_action=1)
    st = o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, 1_700_000_000))["verdict"] & 0xFF
    d = pyoracle.OracleDefrag(fcb_max=2048)
    n = len(lens)
    assert n <= 2048
    a = np.concatenate([hdr.reshape(-1), np.full(dfc.TAIL, dfc.FILL, np.uint8)])
    r = d.batch(a, np.arange(n, dtype=np.uint64) * hdr.shape[1], lens, NOW, full=False)
    d.close()
    frag = st == abi.ST["FRAG"]
    bad = np.nonzero(((r["status"] & 0xFF) != dfc.NOT_FRAG) != frag)[0]
    assert len(bad) == 0, meta["name"][bad[:6]].tolist()
    assert frag.sum() > 100
