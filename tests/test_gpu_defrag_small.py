"""The one-launch kernel for small fragment batches (csrc/ppe_defrag_small.hip) on the GPU: two FCB tables fed the same
batches, one of them created under PPE_DEFRAG_SMALL=0 (every batch on the six launches), and the oracle's sequential
Defrag.

Bar: after every batch both tables' outputs are bit-identical to each other over every word of every output buffer,
the 64 guard entries behind each included (status with the teardrop bit, datagram index, count, lengths, windows,
whole frames, fragment-id lists, and whatever stays unwritten), and equal to the oracle's wherever the ABI defines them;
ppe_defrag_info is the same for all three after every batch; every aging call drops the same ids; and
ppe_defrag_launch_info names the path each batch took."""
import os
import re
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from pktbuild import arena, ip_frag, udp  # noqa: E402
from ppe import Defrag, Engine, synth  # noqa: E402

import defrag_corpus as dfc  # noqa: E402

DEV = torch.device("cuda:0")
NOW = 1_000_000
GUARD = 64
ROOT = Path(__file__).resolve().parent.parent
CUT = int(re.search(r"#define PPE_DEFRAG_SMALL_CUTOFF (\d+)u",
                    (ROOT / "packet-process-engine_amd" / "csrc" / "ppe_internal.h").read_text()).group(1))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


BLOCK = 256   # the kernel's workgroup: the most fragments it holds (PPE_DEFRAG_SMALL=256 takes it up to there)


@contextmanager
def small_env(value):
    old = os.environ.get("PPE_DEFRAG_SMALL")
    os.environ["PPE_DEFRAG_SMALL"] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ["PPE_DEFRAG_SMALL"]
        else:
            os.environ["PPE_DEFRAG_SMALL"] = old


def alloc(g, n, stride):
    """Output tensors for n fragments with GUARD more entries / rows behind each, all filled."""
    out = g.alloc_out(n + GUARD, stride)
    out["n_dgram"] = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
    for v in out.values():
        v.fill_(-7) if v.dtype != torch.uint8 else v.fill_(0xA5)
    return out


def against_oracle(got, ref, n, stride):
    st = got["status"].view(np.uint32)
    bad = np.nonzero(st[:n] != ref["status"])[0]
    assert len(bad) == 0, (f"status: {len(bad)} mismatches, first {bad[:6].tolist()}: gpu={st[bad[:6]].tolist()} "
                           f"ref={ref['status'][bad[:6]].tolist()}")
    nd = ref["n_dgram"]
    assert int(got["n_dgram"][0]) == nd
    assert np.array_equal(got["dgram_of"].view(np.uint32)[:n], ref["dgram_of"])
    assert np.array_equal(got["dgram_len"].view(np.uint32)[:n], ref["dgram_len"])   # 0 past the count
    assert np.array_equal(got["dgram_frags"].view(np.uint64)[:nd], ref["dgram_frags"][:nd])
    for j in range(nd):
        m = int(ref["dgram_len"][j])
        assert np.array_equal(got["dgram_pkt"][j, :m], ref["dgram_pkt"][j, :m]), f"datagram {j} bytes"
        w = np.zeros(stride, np.uint8)
        w[:min(m, stride)] = ref["dgram_pkt"][j, :min(m, stride)]
        assert np.array_equal(got["dgram_hdr"][j], w), f"datagram {j} window"
    # rows past the count and the guard entries: untouched
    assert (got["dgram_hdr"][nd:] == 0xA5).all() and (got["dgram_pkt"][nd:] == 0xA5).all()
    assert (got["dgram_frags"][nd:] == -7).all()
    for k in ("status", "dgram_of", "dgram_len"):
        assert (got[k][n:] == -7).all(), f"{k}: written past n"
    assert (got["n_dgram"][1:] == -7).all()


class Trio:
    """Two HIP FCB tables (small batches in one launch / always six launches) and the oracle's.  upto: the largest
    batch the first table gives the one launch: the cutoff, or with the diagnostic PPE_DEFRAG_SMALL=256 the whole
    workgroup, so the kernel is held to the oracle at every size it can run, whatever cutoff the measurement sets."""

    def __init__(self, eng, stride=128, upto=None, **cfg):
        self.upto = upto or CUT
        if upto:
            with small_env(upto):
                self.s = Defrag(eng, **cfg)
        else:
            self.s = Defrag(eng, **cfg)
        with small_env(0):
            self.x = Defrag(eng, **cfg)
        self.o = pyoracle.OracleDefrag(fcb_max=cfg.get("fcb_max", 0), cache_max=cfg.get("cache_max", 0),
                                       frag_buf=cfg.get("frag_buf_bytes", 0), reasm_buf=cfg.get("reasm_buf_bytes", 0))
        self.stride = stride
        assert self.s.launch_info() == (0, 0) and self.x.launch_info() == (0, 0)

    def close(self):
        self.s.close()
        self.x.close()
        self.o.close()

    @staticmethod
    def dev(a, off, lens, ids):
        return (torch.from_numpy(np.ascontiguousarray(a)).to(DEV),
                torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(DEV),
                torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32)).to(DEV),
                torch.from_numpy(np.ascontiguousarray(ids, np.uint64).view(np.int64)).to(DEV) if ids is not None else None)

    def batch(self, a, off, lens, now, ids=None, stats=True):
        n = len(lens)
        ref = self.o.batch(a, off, lens, now, ids=ids)
        ta, to, tl, ti = self.dev(a, off, lens, ids)
        got = []
        for g in (self.s, self.x):
            out = alloc(g, n, self.stride)
            g.run_torch(ta, to, tl, out, now, ids=ti)
            torch.cuda.synchronize()
            got.append({k: v.cpu().numpy() for k, v in out.items()})
        assert self.s.launch_info() == ((1, 1) if n <= self.upto else (0, 6))
        assert self.x.launch_info() == (0, 6)
        for k in got[0]:
            assert np.array_equal(got[0][k], got[1][k]), f"{k}: one launch != six launches"
        against_oracle(got[0], ref, n, self.stride)
        if stats:
            self.check_stats()
        return got[0], ref

    def age(self, now, timeout=20):
        si, sf = self.s.age(now, timeout)
        xi, xf = self.x.age(now, timeout)
        oi, of = self.o.age(now, timeout)
        assert sf == xf == of
        assert sorted(si.tolist()) == sorted(xi.tolist()) == sorted(oi.tolist())

    def check_stats(self):
        si, xi, os_ = self.s.info(), self.x.info(), self.o.stats()
        assert si == xi
        for k, v in os_.items():
            assert si[k] == v, (k, si[k], v)


def replay(eng, a, o, l, sizes, every_age=3, timeout=20, stride=128, upto=None, **cfg):
    """The stream in consecutive batches of sizes[k % len(sizes)] fragments."""
    t = Trio(eng, stride=stride, upto=upto, **cfg)
    try:
        ids = np.arange(len(l), dtype=np.uint64) * 3 + 11
        b = k = 0
        while b < len(l):
            n = sizes[k % len(sizes)]
            t.batch(a, o[b:b + n], l[b:b + n], NOW + k, ids=ids[b:b + n])
            if (k + 1) % every_age == 0:
                t.age(NOW + k, timeout)
            b += n
            k += 1
        t.age(NOW + 10**6, timeout)
        t.check_stats()
        assert t.s.info()["running"] == 0
    finally:
        t.close()


@pytest.mark.parametrize("n", sorted({1, 2, 63, 64, 65, CUT - 1, CUT, CUT + 1} - {0}))
def test_batch_sizes_around_the_waves_and_the_cutoff(eng, n):
    a, o, l = synth.make_fragment_stream(40 if n < 8 else max(100, int(n * 1.3)), seed=100 + n)
    replay(eng, a, o[:4 * n + 40], l[:4 * n + 40], [n], every_age=2)


@pytest.mark.parametrize("n", [5, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_batch_sizes_up_to_the_workgroup(eng, n):
    """The kernel at the sizes its workgroup holds, past the cutoff in force (PPE_DEFRAG_SMALL=256)."""
    a, o, l = synth.make_fragment_stream(max(100, int(n * 1.3)), seed=200 + n)
    replay(eng, a, o[:4 * n + 40], l[:4 * n + 40], [n], every_age=2, upto=BLOCK)


@pytest.mark.parametrize("upto", [None, BLOCK], ids=["cutoff", "workgroup"])
@pytest.mark.parametrize("cfg", list(dfc.CONFIGS))
def test_corpus_back_to_back_at_the_cutoff(eng, cfg, upto):
    """The config's cases back to back, cut into batches of the cutoff (chains cross the batches wherever the cut
    falls), with the corpus's hand-derived statuses."""
    cs = dfc.of_config(dfc.cases(), cfg)
    a, bts = dfc.layout(cs, dict(dfc.arrangements(cs))["together"], 4)
    off, lens, gid, want = bts[0]
    t = Trio(eng, upto=upto, **dict(dfc.CONFIGS[cfg], max_batch=1024))
    step = upto or CUT
    try:
        for k, b in enumerate(range(0, len(lens), step)):
            sl = slice(b, b + step)
            _, ref = t.batch(a, off[sl], lens[sl], NOW + k, ids=gid[sl] * np.uint64(3) + np.uint64(11))
            assert np.array_equal(ref["status"], want[sl])
        t.age(NOW + 10**6)
        t.check_stats()
    finally:
        t.close()


@pytest.mark.parametrize("cfg", list(dfc.CONFIGS))
def test_corpus_one_fragment_of_every_chain_per_batch(eng, cfg):
    """Batch k holds the k-th fragment of every chain (at most the workgroup's 256 per batch, every batch in one
    launch: PPE_DEFRAG_SMALL=256), with an aging call after each:
    every chain is continued from the store slots and the FCB's id list, and every table rebuild is followed by small
    batches."""
    cs = dfc.of_config(dfc.cases(), cfg)
    a, bts = dfc.layout(cs, dict(dfc.arrangements(cs))["columns"], 1)
    t = Trio(eng, upto=BLOCK, **dict(dfc.CONFIGS[cfg], max_batch=1024))
    try:
        k = 0
        for off, lens, gid, want in bts:
            for b in range(0, len(lens), BLOCK):
                sl = slice(b, b + BLOCK)
                _, ref = t.batch(a, off[sl], lens[sl], NOW + k, ids=gid[sl] * np.uint64(3) + np.uint64(11), stats=False)
                assert np.array_equal(ref["status"], want[sl])
                t.age(NOW + k, dfc.NEVER)
                k += 1
        t.check_stats()
        t.age(NOW + 10**6)
        t.check_stats()
    finally:
        t.close()


def test_more_creators_than_fcbs_in_one_batch(eng):
    """fcb_max 3 and eight new keys in one 20-fragment batch: the first three creators in index order get FCBs."""
    S, D = 0x0A000001, 0x0A000002
    l4 = udp(1, 2, bytes(range(24)))
    frames = []
    for f in range(3):
        for k in range(8):
            if (k + f) % 5 != 4:
                frames.append(ip_frag(17, S + k, D, 50 + k, 8 * f, True, l4[8 * f:8 * f + 8]))
    a, o, l = arena(frames[:20])
    t = Trio(eng, upto=BLOCK, fcb_max=3, max_batch=64)
    try:
        got, ref = t.batch(a, o, l, NOW)
        creators = []   # the keys in the order of their first fragments: the first three get FCBs
        for fr in frames[:20]:
            if fr[26:30] not in creators:
                creators.append(fr[26:30])
        assert len(creators) == 8
        want = [0 if fr[26:30] in creators[:3] else 3 for fr in frames[:20]]
        assert ref["status"].tolist() == want
        t.batch(a, o, l, NOW + 1)       # the same keys again: the three FCBs found, the others full again
        t.age(NOW + 100)
        t.batch(a, o[::-1].copy(), l[::-1].copy(), NOW + 101)
    finally:
        t.close()


@pytest.mark.parametrize("cm", [3, 16])
def test_cache_max(eng, cm):
    a, o, l = synth.make_fragment_stream(260, seed=10 + cm, jumbo=0.1 if cm == 16 else 0.0)
    replay(eng, a, o, l, [200, 7, 64, 3], upto=BLOCK, cache_max=cm, reasm_buf_bytes=16384 if cm == 16 else 0, fcb_max=40 if cm == 3 else 0)


def test_a_group_past_its_slots_in_one_small_batch(eng):
    """Datagrams cut into 12 / 15 / 16 / 17 / 40 eight-byte fragments plus duplicates, shuffled into one batch
    that one workgroup holds (PPE_DEFRAG_SMALL=256: the measured cutoff lies below a group's 15 slots): groups with more members than the 15 slots are stepped from gkey, with cache_max 8 and 16."""
    rng = np.random.default_rng(77)
    S, D = 0x0A000001, 0x0A0000FE
    frames = []
    for k, nf in enumerate([12, 15, 16, 17, 40]):
        l4 = udp(1000 + k, 53, rng.integers(0, 256, 8 * nf - 8, dtype=np.uint8).tobytes())
        frs = [ip_frag(17, S + k, D, 100 + k, 8 * f, f < nf - 1, l4[8 * f:8 * f + 8]) for f in range(nf)]
        frames += frs + [frs[f] for f in rng.choice(nf, 4)]
    frames = [frames[i] for i in rng.permutation(len(frames))]
    assert 64 < len(frames) <= BLOCK
    a, o, l = arena(frames)
    for cm in (8, 16):
        t = Trio(eng, upto=BLOCK, cache_max=cm, max_batch=256)
        try:
            t.batch(a, o, l, NOW)
            t.batch(a, o, l, NOW + 1)   # every FCB found in the table this time
        finally:
            t.close()


def test_byte_aligned_frames(eng):
    a, o, l = synth.make_fragment_stream(200, seed=9, align=1)
    replay(eng, a, o, l, [CUT, 33, 1, BLOCK], upto=BLOCK)


def test_window_64(eng):
    a, o, l = synth.make_fragment_stream(200, seed=11)
    replay(eng, a, o, l, [CUT, 5, 100], stride=64, upto=BLOCK)


def test_small_and_large_batches_alternate_on_one_table(eng):
    a, o, l = synth.make_fragment_stream(6000, seed=12)
    assert len(l) >= 16400
    replay(eng, a, o[:16400], l[:16400], [100, 8000, CUT, 8000, 1], every_age=2, upto=BLOCK, max_batch=8192)


def test_300_small_batches_queued_without_a_synchronise(eng):
    """300 batches of 1-8 fragments enqueued back to back on each table, one synchronise at the end: every batch's
    outputs against the oracle's, and the two tables' against each other."""
    a, o, l = synth.make_fragment_stream(900, seed=13)
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, CUT + 1, 300)
    assert sizes.sum() <= len(l)
    ids = np.arange(len(l), dtype=np.uint64) * 3 + 11
    t = Trio(eng, max_batch=64)
    try:
        ta, to, tl, ti = t.dev(a, o, l, ids)
        outs = []
        for g in (t.s, t.x):
            mine, b = [], 0
            for n in sizes:
                out = alloc(g, int(n), 128)
                g.run_torch(ta, to[b:b + n], tl[b:b + n], out, NOW, ids=ti[b:b + n])
                mine.append(out)
                b += int(n)
            outs.append(mine)
        torch.cuda.synchronize()
        assert t.s.launch_info() == (1, 1) and t.x.launch_info() == (0, 6)
        b = 0
        for k, n in enumerate(sizes):
            n = int(n)
            ref = t.o.batch(a, o[b:b + n], l[b:b + n], NOW, ids=ids[b:b + n])
            got = [{key: v.cpu().numpy() for key, v in outs[w][k].items()} for w in (0, 1)]
            for key in got[0]:
                assert np.array_equal(got[0][key], got[1][key]), (k, key)
            against_oracle(got[0], ref, n, 128)
            b += n
        t.check_stats()
        t.age(NOW + 100)
        t.check_stats()
    finally:
        t.close()
