"""The reassembly edge corpus (tests/defrag_corpus.py) through ppe_defrag / ppe_defrag_age on the GPU: every table
config, the cases back to back, interleaved and one fragment of every chain per batch (so each chain is continued from
the store slots and the FCB's id list), frames on 4-byte and on byte boundaries, both window strides, with and without
caller ids; then aging on the clock's edges, the optional outputs absent, and the decoder's own edge corpus.

Bar: bit-exact against the oracle's sequential Defrag through DfPair (tests/test_gpu_defrag.py: status with the
teardrop bit, datagram index, count, lengths, bytes, window, fragment ids, untouched rows past the count, the aging
result, the counters), and the oracle's statuses equal to the corpus's hand-derived ones, so a failure names its case.
The arenas carry 0xA5 between the frames and behind the last, so a read past a frame changes what is parsed."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from pktbuild import ip_frag  # noqa: E402
from ppe import Defrag, Engine, abi, synth  # noqa: E402

import defrag_corpus as dfc  # noqa: E402
from test_gpu_defrag import DEV, NOW, DfPair  # noqa: E402

CASES = dfc.cases()
MAXB = 1024          # max_batch of the corpus's tables (a sequence's largest batch is a few hundred fragments)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@lru_cache(maxsize=None)
def sequence(group, arrangement, align):
    """(cases, arena, batches, fcb_max) of one arrangement of a config's cases, or of the FCB_FULL group."""
    if group == "fcb_full":
        cs, fcb_max, want = dfc.fcb_full_group(CASES)
    else:
        cs, fcb_max, want = dfc.of_config(CASES, group), None, None
    a, bts = dfc.layout(cs, dict(dfc.arrangements(cs))[arrangement], align, want)
    return cs, a, bts, fcb_max


def names(cs, gids):
    base = np.cumsum([len(c.frames) for c in cs])
    return [f"{cs[int(np.searchsorted(base, g, 'right'))].name}[{int(g)}]" for g in gids]


def play(eng, group, arrangement, align, stride, ids=True):
    cs, a, bts, fcb_max = sequence(group, arrangement, align)
    cfg = dict(dfc.CONFIGS["default" if group == "fcb_full" else group], max_batch=MAXB)
    if fcb_max:
        cfg["fcb_max"] = fcb_max
    p = DfPair(eng, stride=stride, **cfg)
    try:
        for k, (off, lens, gid, want) in enumerate(bts):
            assert len(lens) <= MAXB
            try:
                _, ref = p.batch(a, off, lens, NOW + k, ids=gid * np.uint64(3) + np.uint64(11) if ids else None)
            except AssertionError as e:   # name the cases behind DfPair's fragment and datagram indices
                who = names(cs, gid)
                raise AssertionError(f"{e}\nbatch {k}: datagrams, in order: "
                                     f"{[w for w, s in zip(who, want) if s == dfc.REASM]}\nfragments, in order: {who}") from e
            bad = np.nonzero(ref["status"] != want)[0]
            assert len(bad) == 0, (names(cs, gid[bad[:6]]), ref["status"][bad[:6]].tolist(), want[bad[:6]].tolist())
            if len(bts) > 1:
                p.age(NOW + k, dfc.NEVER)
        p.check_stats()
        p.age(NOW + 10**6, 20)   # everything still held is dropped: the same ids as the oracle's
        p.check_stats()
        assert p.g.info()["running"] == 0
    finally:
        p.close()


@pytest.mark.parametrize("stride", [64, 128])
@pytest.mark.parametrize("align", [4, 1])
@pytest.mark.parametrize("arrangement", ["together", "interleaved", "columns"])
@pytest.mark.parametrize("cfg", list(dfc.CONFIGS))
def test_corpus_vs_oracle(eng, cfg, arrangement, align, stride):
    play(eng, cfg, arrangement, align, stride)


@pytest.mark.parametrize("align", [4, 1])
@pytest.mark.parametrize("cfg", list(dfc.CONFIGS))
def test_columns_without_ids(eng, cfg, align):
    """ids = NULL: a fragment of an earlier batch is named by its index in that batch, in the datagram's fragment list
    and in the aging's dropped list."""
    play(eng, cfg, "columns", align, 128, ids=False)


@pytest.mark.parametrize("arrangement", ["together", "interleaved", "columns"])
def test_fcb_full_group(eng, arrangement):
    """fcb_max two short of the keys: the last two creators in index order fail, on their later fragments too."""
    play(eng, "fcb_full", arrangement, 1, 128)


# ---- aging on the clock's edges (Frag_defrag_timeout, decode-defrag.c:519-520: now > cycle && now - cycle > timeout)
S, D = 0x0B000001, 0x0B000002
L4 = dfc.pat(32, 7)
CHAIN = [(ip_frag(17, S, D, 9, 8 * k, k < 3, L4[8 * k:8 * k + 8]), 42) for k in range(4)]


def feed(p, frames, now, ids, want):
    a, off, lens = dfc.arena(frames, 1)
    got, ref = p.batch(a, off, lens, now, ids=np.asarray(ids, np.uint64))
    assert ref["status"].tolist() == want
    return got


def age(p, now, timeout, freed, dropped):
    """DfPair.age (GPU == oracle) and the hand-derived answer."""
    gi, gf = p.g.age(now, timeout)
    oi, of = p.o.age(now, timeout)
    assert (gf, sorted(gi.tolist())) == (of, sorted(oi.tolist())) == (freed, sorted(dropped))


def test_age_at_the_timeout_keeps_the_chain(eng):
    p = DfPair(eng, max_batch=MAXB)
    try:
        feed(p, CHAIN[:2], NOW, [70, 71], [0, 0])
        age(p, NOW - 5, 0, 0, [])          # now < the FCB's time
        age(p, NOW, 0, 0, [])              # timeout 0 at the FCB's own second: now > cycle fails
        age(p, NOW + 20, 20, 0, [])        # idle == timeout
        got = feed(p, CHAIN[2:], NOW + 20, [72, 73], [0, 1])   # the second half completes it
        assert got["dgram_frags"].view(np.uint64)[0, :4].tolist() == [70, 71, 72, 73]
        p.check_stats()
    finally:
        p.close()


def test_age_one_past_the_timeout_drops_it(eng):
    p = DfPair(eng, max_batch=MAXB)
    try:
        feed(p, CHAIN[:2], NOW, [70, 71], [0, 0])
        age(p, NOW + 21, 20, 1, [70, 71])  # idle == timeout + 1
        feed(p, CHAIN[2:], NOW + 21, [72, 73], [0, 0])         # a new FCB: no first fragment, stays cached
        assert p.g.info()["new_fcb"] == 2
        age(p, NOW + 22, 0, 1, [72, 73])   # timeout 0, one second on
        p.check_stats()
    finally:
        p.close()


def test_a_rejected_fragment_refreshes_its_fcb(eng):
    """FragFind stamps the FCB before Frag_defrag_process rejects the fragment (:137)."""
    p = DfPair(eng, max_batch=MAXB)
    try:
        feed(p, CHAIN[:1], NOW, [70], [0])
        feed(p, CHAIN[:1], NOW + 15, [71], [abi.DF["DEFRAG_ERR"] | abi.DF_TEARDROP])
        age(p, NOW + 21, 20, 0, [])        # 6 s after the duplicate
        age(p, NOW + 35, 20, 0, [])        # idle == timeout since the duplicate
        age(p, NOW + 36, 20, 1, [70])
        p.check_stats()
    finally:
        p.close()


def test_an_fcb_full_fragment_refreshes_nothing(eng):
    """fcb_create fails before any FCB is stamped (:75-82): the one FCB ages from its own fragment's time, and the
    refused key holds no record afterwards."""
    other = [(ip_frag(17, S + 1, D, 9, 0, True, L4[:8]), 42)]
    p = DfPair(eng, fcb_max=1, max_batch=MAXB)
    try:
        feed(p, CHAIN[:1], NOW, [70], [0])
        feed(p, other, NOW + 15, [80], [abi.DF["FCB_FULL"]])
        age(p, NOW + 20, 20, 0, [])
        age(p, NOW + 21, 20, 1, [70])
        feed(p, other, NOW + 22, [81], [0])
        p.check_stats()
    finally:
        p.close()


# ---- optional outputs ------------------------------------------------------------------------------------------------
OPTIONAL = ("dgram_of", "dgram_pkt", "dgram_frags", "n_dgram")


@pytest.mark.parametrize("absent", [(k,) for k in OPTIONAL] + [OPTIONAL], ids=lambda t: "+".join(t))
def test_optional_outputs_absent(eng, absent):
    """The interleaved default batch with optional output pointers NULL: the remaining outputs equal the full run's
    (which test_corpus_vs_oracle holds to the oracle)."""
    cs, a, bts, _ = sequence("default", "interleaved", 1)
    off, lens, gid, _ = bts[0]
    n = len(lens)
    ta = torch.from_numpy(a).to(DEV)
    to = torch.from_numpy(off.view(np.int64)).to(DEV)
    tl = torch.from_numpy(lens.view(np.int32)).to(DEV)
    ti = torch.from_numpy(gid.view(np.int64)).to(DEV)
    res = []
    for drop in ((), absent):
        g = Defrag(eng, **dict(dfc.CONFIGS["default"], max_batch=MAXB))
        try:
            out = g.alloc_out(n, 128)
            for v in out.values():
                v.fill_(-7) if v.dtype != torch.uint8 else v.fill_(0xA5)
            for k in drop:
                out[k] = None
            g.run_torch(ta, to, tl, out, NOW, ids=ti)
            torch.cuda.synchronize()
            res.append(({k: v.cpu().numpy() for k, v in out.items() if v is not None}, g.info()))
        finally:
            g.close()
    (full, finfo), (part, pinfo) = res
    nd = int(full["n_dgram"][0])
    assert nd > 20 and set(part) == set(full) - set(absent) and pinfo == finfo
    for k, v in part.items():
        if k == "dgram_pkt":
            for j in range(nd):
                m = int(full["dgram_len"][j])
                assert np.array_equal(v[j, :m], full[k][j, :m]), (k, j)
            assert (v[nd:] == 0xA5).all()
        else:
            assert np.array_equal(v, full[k]), k


# ---- the decoder's edge corpus ------------------------------------------------------------------------------------
def test_decode_corpus_fragments(eng):
    """The frames of tests/decode_corpus.py through ppe_defrag: NOT_FRAG exactly where the decoder's oracle does not
    report status FRAG, everything else as OracleDefrag (DfPair)."""
    import decode_corpus as dc
    rules = synth.make_rules(256, seed=256)
    hdr, lens, meta = dc.corpus(rules)
    o = pyoracle.Oracle(rules, default_action=1)
    frag = (o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, 1_700_000_000))["verdict"] & 0xFF) == abi.ST["FRAG"]
    n = len(lens)
    a = np.concatenate([hdr.reshape(-1), np.full(dfc.TAIL, dfc.FILL, np.uint8)])
    p = DfPair(eng, fcb_max=2048, max_batch=2048)
    try:
        got, _ = p.batch(a, np.arange(n, dtype=np.uint64) * np.uint64(hdr.shape[1]), lens, NOW)
        st = got["status"].view(np.uint32) & 0xFF
        bad = np.nonzero((st != abi.DF["NOT_FRAG"]) != frag)[0]
        assert len(bad) == 0, meta["name"][bad[:6]].tolist()
        assert frag.sum() > 100
        p.check_stats()
    finally:
        p.close()
