"""A deterministic corpus of IPv4 fragment chains on both sides of every comparator of the reassembly (helper, no
tests): the parse before Defrag, the state machine of Frag_defrag_process, the buffer and count limits, and the bytes
Frag_defrag_reasm assembles.  Every frame is built from explicit bytes (tests/pktbuild.py).

A case is a list of frames under one FCB key of its own (sip, dip, ip_id), the table config it needs (CONFIGS) and its
expected status list `want`, derived by hand from dataplane/src/decode/decode-defrag.c (the lines are named beside
each case; the oracle cannot be pinned to reference outputs, so these answers pin it, as tests/test_oracle_defrag.py
does).  FCBs interact only through fcb_max, so a case's statuses are the same alone and in any arrangement of the
corpus (arrangements()): together, interleaved, or one fragment of every chain per batch.

What the reference's state machine makes unreachable: every accepted fragment is inserted between a predecessor that
ends at or before its offset and a successor that starts at or after its end (decode-defrag.c:350-366), so a chain is
always sorted and disjoint, and it completes only when it tiles [0, total) exactly (:383-384).  Fragment offsets are
multiples of 8, so every later fragment of a completed chain starts at l2 + ihl*4 + 8k of the output: `dst0 & 3` of a
copied segment is always 2 (the head frame's own start is 0).  What does vary, and the corpus covers in full, is the
segment's end (end & 3: the bytes behind its last whole dword) and, with byte-aligned frames, the source phase."""
import numpy as np

from pktbuild import ip_frag

CACHED, REASM, SETUP_ERR, FCB_FULL, HW2SW_ERR, DELETED, CACHE_FULL, DEFRAG_ERR, NOT_FRAG = range(9)
TEAR = 0x100
FILL = 0xA5                     # between the frames and behind the last: a read past a frame changes what is parsed
TAIL = 64                       # filler bytes behind the last frame
NEVER = 100_000                 # an aging timeout no sequence reaches

# Defrag(engine, **CONFIGS[name]); oracle_cfg(name) for OracleDefrag.  tight: three fragments per FCB, and a
# reassembly buffer a 64-byte datagram fills exactly (64 + 14 + 20); not a multiple of 4, so datagram rows start at
# odd dword phases
CONFIGS = {
    "default": dict(fcb_max=1024, cache_max=8, frag_buf_bytes=2024, reasm_buf_bytes=8168),
    "cm16": dict(fcb_max=1024, cache_max=16, frag_buf_bytes=2024, reasm_buf_bytes=8168),
    "tight": dict(fcb_max=1024, cache_max=3, frag_buf_bytes=2024, reasm_buf_bytes=98),
}
TAGS = {"untagged": dict(), "tag8100": dict(vlan_tag=True), "tag9100": dict(vlan_tag=True, etype=0x9100)}


def oracle_cfg(name, fcb_max=None):
    c = CONFIGS[name]
    return dict(fcb_max=fcb_max or c["fcb_max"], cache_max=c["cache_max"], frag_buf=c["frag_buf_bytes"],
                reasm_buf=c["reasm_buf_bytes"])


def pat(n, salt):
    """n payload bytes, different for every salt and without long runs of one value."""
    return bytes((i * 37 + salt * 101 + (i >> 4) * 3 + 7) & 0xFF for i in range(n))


class Case:
    """frames: (bytes, wire length): the bytes go into the arena whole (bytes past the wire length lie behind the frame
    like a crafted next frame); want: the status word of each frame; cols: the batch of each frame in the `columns`
    arrangement; payload: the L4 bytes a non-ICMP datagram must carry, in offset order."""

    def __init__(self, name, cfg, family, key):
        self.name, self.cfg, self.family, self.key = name, cfg, family, key
        self.frames, self.want, self.cols, self.payload = [], [], [], None

    def add(self, want, proto, off, mf, chunk, wire=None, cut=False, col=None, **kw):
        fr = ip_frag(proto, self.key[0], self.key[1], self.key[2], off, mf, chunk, **kw)
        n = len(fr) if wire is None else wire
        self.frames.append((fr[:n] if cut else fr, n))
        self.want.append(want)
        self.cols.append(len(self.cols) if col is None else col)
        return self


class _Builder:
    def __init__(self):
        self.cases = []

    def case(self, name, cfg="default", family="B"):
        k = len(self.cases)
        c = Case(name, cfg, family, (0x0A000001 + k, 0xC0A80001 + 3 * k, (0x0101 * (k + 1)) & 0xFFFF))
        self.cases.append(c)
        return c


# ---- family A: the parse, one frame each ----------------------------------------------------------------------------
# What DecodeEthernet / DecodeVLAN / DecodeIPV4 drop before Defrag is NOT_FRAG; every rejected row sits beside a row
# that differs in the one field and is accepted (CACHED: Defrag :467-482 creates the FCB, Frag_defrag_process :383-393
# caches the lone fragment).
def _family_a(b):
    for tname, tkw in TAGS.items():
        l2 = 18 if tkw else 14

        def one(name, want, chunk=pat(16, 1), off=0, mf=True, proto=17, **kw):
            b.case(f"A/{tname}/{name}", family="A").add(want, proto, off, mf, chunk, **dict(tkw, **kw))

        one("ok", CACHED)
        # the low 16 bits of the length against 14, l2 + 20 and the header: the bytes behind the short frame are the
        # rest of a valid fragment (ip_len 20, so any longer wire length is accepted), or the filler (cut)
        for n in (13, 14) + ((17, 18) if tkw else ()) + (l2 + 19, l2 + 20):
            one(f"len{n}", NOT_FRAG, wire=n, ip_len=20)
            one(f"len{n}_cut", NOT_FRAG, wire=n, ip_len=20, cut=True)
        one(f"len{l2 + 21}", CACHED, wire=l2 + 21, ip_len=20)               # frag_len 1
        one(f"len{l2 + 21}_cut", CACHED, wire=l2 + 21, ip_len=20, cut=True)
        one("dmac0", NOT_FRAG, dmac=bytes(6))
        one("smac0", NOT_FRAG, smac=bytes(6))
        one("dmac_low0", CACHED, dmac=bytes([2, 0, 0, 0, 0, 0]))           # only an all-zero address is dropped
        one("smac_high0", CACHED, smac=bytes([0, 0, 0, 0, 0, 9]))
        if tkw:
            one("inner86dd", NOT_FRAG, inner=0x86DD)
            one("inner8100", NOT_FRAG, inner=0x8100)                        # a second tag never reaches IPv4
            one("etype88a8", NOT_FRAG, etype=0x88A8)                        # not a tag here
        else:
            one("etype88a8", NOT_FRAG, etype=0x88A8)
            one("etype0806", NOT_FRAG, etype=0x0806)
        one("ver5", NOT_FRAG, ver=5)
        one("ihl4", NOT_FRAG, ihl=4)
        one("ihl15", CACHED, ihl=15)
        one("iplen_lt_hlen", NOT_FRAG, ip_len=19)
        one("iplen_eq_hlen", CACHED, ip_len=20)
        one("iplen_l3+1", NOT_FRAG, ip_len=20 + 16 + 1)
        one("iplen_lt_l3", CACHED, pad=5)                                   # the padding counts in frag_len
        for offw, want in ((0x0000, NOT_FRAG), (0x4000, NOT_FRAG), (0x8000, NOT_FRAG), (0xC000, NOT_FRAG),
                           (0x2000, CACHED), (0x6000, CACHED), (0x0001, CACHED), (0x1FFF, CACHED)):
            one(f"off{offw:04x}", want, offw=offw)
        one("proto89", NOT_FRAG, proto=89)
        one("proto88", CACHED, proto=88)
        one("flen0", NOT_FRAG, chunk=b"")
        one("flen0_ihl6", NOT_FRAG, chunk=b"", ihl=6)
        # bits above 16: parsed by the low 16 bits (Decode, decode.c:25), the FCB created (:467-482), then the whole
        # length fails PACKET_HW2SW (:415-420)
        one("len+65536", HW2SW_ERR, wire=len(ip_frag(17, 0, 0, 0, 0, True, pat(16, 1), **tkw)) + 65536)


# ---- family B: the state machine -----------------------------------------------------------------------------------
def _family_b(b):
    k = [100]

    def l4(n):
        k[0] += 1
        return pat(n, k[0])

    # in order: tail append (:330-335), completion (:383-388), Frag_defrag_reasm (:241-256)
    p = l4(40)
    c = b.case("B/in_order")
    c.add(CACHED, 17, 0, True, p[:16]).add(CACHED, 17, 16, True, p[16:32]).add(REASM, 17, 32, False, p[32:])
    c.payload = p
    # two reversed: final first (:308-314), then offset 0: the scan (:337-342) stops at the final one (frag_len 8 >= 0)
    p = l4(16)
    c = b.case("B/two_reversed")
    c.add(CACHED, 17, 8, False, p[8:]).add(REASM, 17, 0, True, p[:8])
    c.payload = p
    # middle last: the scan compares the chained frag_len with the new offset (:339): offset 16 stops at the head
    # (frag_len 16 >= 16) and then overlaps it as `next` (:359-366)
    p = l4(48)
    b.case("B/middle_last_teardrop").add(CACHED, 17, 0, True, p[:16]).add(CACHED, 17, 32, False, p[32:]) \
        .add(DEFRAG_ERR | TEAR, 17, 16, True, p[16:32])
    # duplicate: tail offset 0 is not < 0 (:331), the scan stops at the head, 0 - 16 < 0 (:360-361)
    p = l4(16)
    b.case("B/duplicate").add(CACHED, 17, 0, True, p).add(DEFRAG_ERR | TEAR, 17, 0, True, p)
    # a final fragment that ends before the total (:310): no teardrop
    p = l4(32)
    b.case("B/short_final").add(CACHED, 17, 0, True, p).add(DEFRAG_ERR, 17, 16, False, p[16:24])
    # a second final (:310, LAST_IN)
    p = l4(48)
    b.case("B/second_final").add(CACHED, 17, 32, False, p[32:]).add(DEFRAG_ERR, 17, 40, False, p[40:])
    # a rejected non-final still raises the total (:317-322 run before the overlap checks): end 40 > 16, then the
    # overlap with the tail (:350-357); the final at end 32 < 40 can no longer be accepted (:310)
    p = l4(32)
    b.case("B/non_final_extends").add(CACHED, 17, 0, True, p[:16]).add(DEFRAG_ERR | TEAR, 17, 8, True, bytes(32)) \
        .add(DEFRAG_ERR, 17, 16, False, p[16:])
    # a completed FCB answers DELETE (:276, :424-429) until the timer frees it (:519-520): the duplicate shares the
    # completing fragment's batch in `columns`, where every batch is followed by an aging call
    p = l4(16)
    c = b.case("B/deleted_until_aged")
    c.add(CACHED, 17, 0, True, p[:8]).add(REASM, 17, 8, False, p[8:]).add(DELETED, 17, 0, True, p[:8], col=1)
    c.payload = p
    # reverse arrival that completes: P(24, 16, final), X(8, 8), Y(0, 8), Z(16, 8).  X: tail offset 24 >= 8, P's
    # frag_len 16 >= 8 -> before P.  Y: X's frag_len 8 >= 0 -> before X.  Z: Y 8 < 16, X 8 < 16, P 16 >= 16 -> between
    # X and P, 8 + 8 - 16 = 0 and 24 - 24 = 0 (:350-366).  meat 40 == total 40 (:383-384)
    p = l4(40)
    c = b.case("B/reverse_completes")
    c.add(CACHED, 17, 24, False, p[24:]).add(CACHED, 17, 8, True, p[8:16]).add(CACHED, 17, 0, True, p[:8]) \
        .add(REASM, 17, 16, True, p[16:24])
    c.payload = p
    # a non-final fragment padded by 3 B has frag_len 19 (L3 length - ihl*4): 0 + 19 - 16 > 0 (:351-352)
    p = l4(32)
    b.case("B/padded_non_final").add(CACHED, 17, 0, True, p[:16], pad=3).add(DEFRAG_ERR | TEAR, 17, 16, False, p[16:])
    # a final at offset 65,528 with 16 B: end 65,544 does not fit 16 bits.  The head at 0 goes before it (the scan:
    # 16 >= 0; 65,528 - 8 >= 0) and stays cached (meat 24); a second final is refused (:310)
    p = l4(16)
    b.case("B/end_past_65535").add(CACHED, 17, 65528, False, p).add(CACHED, 17, 0, True, p[:8]) \
        .add(DEFRAG_ERR, 17, 32, False, p[8:])
    # ip4_frag_match ignores the protocol (:115-120); the head arrives last and replaces chain position 0.
    # UDP tail, then an ICMP head: Frag_defrag_setup / _reasm take the ICMP branch by the head (:175-178, :257-265):
    # the head frame only, pkt_totallen summed: 50 + 8
    p = l4(24)
    b.case("B/udp_tail_icmp_head").add(CACHED, 17, 16, False, p[16:]).add(REASM, 1, 0, True, p[:16])
    # ICMP tail, then a UDP head: the full copy and the header patch (:244-256)
    p = l4(24)
    c = b.case("B/icmp_tail_udp_head")
    c.add(CACHED, 1, 16, False, p[16:]).add(REASM, 17, 0, True, p[:16])
    c.payload = p

    # cm16: the chain as sixteen 4-bit positions
    # fragments 1..15 of sixteen in order (appends, :330-335), then fragment 0: the scan stops at the first (8 >= 0),
    # an insert at position 0 with 15 chained; meat 128 == total 128
    p = l4(128)
    c = b.case("B/cm16_insert_at_0", cfg="cm16")
    for f in range(1, 16):
        c.add(CACHED, 17, 8 * f, f < 15, p[8 * f:8 * f + 8])
    c.add(REASM, 17, 0, True, p[:8])
    c.payload = p
    # fourteen fragments at 0..104, the final (120, 120), then (112, 8): the scan passes the fourteen (8 < 112) and
    # stops at the final (120 >= 112): an insert at position 14 with 15 chained; 104 + 8 - 112 = 0, 120 - 120 = 0;
    # meat 14 * 8 + 120 + 8 == total 240
    p = l4(240)
    c = b.case("B/cm16_insert_at_14", cfg="cm16")
    for f in range(14):
        c.add(CACHED, 17, 8 * f, True, p[8 * f:8 * f + 8])
    c.add(CACHED, 17, 120, False, p[120:]).add(REASM, 17, 112, True, p[112:120])
    c.payload = p
    # a plain append to 16, then cache_num >= defrag_cache_max (:431-439)
    p = l4(136)
    c = b.case("B/cm16_append_17", cfg="cm16")
    for f in range(17):
        c.add(CACHED if f < 16 else CACHE_FULL, 17, 8 * f, True, p[8 * f:8 * f + 8])


# ---- family C: limits -------------------------------------------------------------------------------------------------
def _family_c(b):
    # PACKET_HW2SW copies into a 2,024-byte slice (:415-420): 2,024 fits, 2,025 does not, after Defrag created the
    # FCB (:467-482): its next fragment finds the FCB empty and is cached
    b.case("C/frame_2024", family="C").add(CACHED, 17, 0, True, pat(2024 - 34, 40))
    b.case("C/frame_2025", family="C").add(HW2SW_ERR, 17, 0, True, pat(2025 - 34, 41)) \
        .add(CACHED, 17, 2000, True, pat(8, 42))
    # Frag_defrag_setup (:181-189): total + L2 + ihl*4 against the 8,168-byte slice: 8,134 + 34 fits
    p = pat(8135, 43)
    c = b.case("C/reasm_fits", family="C")
    for f in range(4):
        c.add(CACHED, 17, 1632 * f, True, p[1632 * f:1632 * f + 1632])
    c.add(REASM, 17, 6528, False, p[6528:8134])
    c.payload = p[:8134]
    # one more byte: STAT_FRAG_SETUP_ERR (:238-239, :281-283) with the fragment already chained (:369-379); the chain
    # stays, so a duplicate is a teardrop (:359-366) and aging drops all five held fragments (:538-544)
    c = b.case("C/reasm_one_more", family="C")
    for f in range(4):
        c.add(CACHED, 17, 1632 * f, True, p[1632 * f:1632 * f + 1632])
    c.add(SETUP_ERR, 17, 6528, False, p[6528:8135]).add(DEFRAG_ERR | TEAR, 17, 0, True, p[:1632])

    # tight: reasm_buf 98, cache_max 3
    p = pat(65, 44)
    c = b.case("C/tight_fits", cfg="tight", family="C")           # 64 + 34 == 98
    c.add(CACHED, 17, 0, True, p[:32]).add(REASM, 17, 32, False, p[32:64])
    c.payload = p[:64]
    b.case("C/tight_one_more", cfg="tight", family="C").add(CACHED, 17, 0, True, p[:32]) \
        .add(SETUP_ERR, 17, 32, False, p[32:65]).add(DEFRAG_ERR | TEAR, 17, 0, True, p[:32])
    p = pat(32, 45)
    c = b.case("C/tight_cache_exact", cfg="tight", family="C")   # the third fragment is accepted and completes
    c.add(CACHED, 17, 0, True, p[:8]).add(CACHED, 17, 8, True, p[8:16]).add(REASM, 17, 16, False, p[16:24])
    c.payload = p[:24]
    c = b.case("C/tight_cache_full", cfg="tight", family="C")    # cache_num 3 >= 3 (:431-439)
    c.add(CACHED, 17, 0, True, p[:8]).add(CACHED, 17, 8, True, p[8:16]).add(CACHED, 17, 16, True, p[16:24]) \
        .add(CACHE_FULL, 17, 24, False, p[24:])
    # the buffer check reads the head that is chained when the datagram completes (:175-182), also when the head
    # arrived last, in a later batch than the fragment it displaces from position 0
    t15 = dict(vlan_tag=True, ihl=15)                             # L2 + ihl*4 = 78, against the plain 34
    p = pat(72, 46)
    # a UDP tail (tagged, ihl 15), then an ICMP head: 1,000 bytes, always there (:175-178); by the tail: 24 + 78 > 98
    b.case("C/tight_icmp_head_last", cfg="tight", family="C").add(CACHED, 17, 16, False, p[16:24], **t15) \
        .add(REASM, 1, 0, True, p[:16])
    # an ICMP tail, then a UDP head: 72 + 34 > 98
    b.case("C/tight_udp_head_last", cfg="tight", family="C").add(CACHED, 1, 32, False, p[32:72]) \
        .add(SETUP_ERR, 17, 0, True, p[:32])
    # a tagged ihl-15 tail, then a plain head: 64 + 34 == 98 fits (by the tail: 64 + 78)
    c = b.case("C/tight_plain_head_last", cfg="tight", family="C")
    c.add(CACHED, 17, 32, False, p[32:64], **t15).add(REASM, 17, 0, True, p[:32])
    c.payload = p[:64]
    # a plain tail, then a tagged ihl-15 head: 24 + 78 > 98 (by the tail: 24 + 34)
    b.case("C/tight_tagged_head_last", cfg="tight", family="C").add(CACHED, 17, 16, False, p[16:24]) \
        .add(SETUP_ERR, 17, 0, True, p[:16], **t15)


# ---- family D: assembled bytes --------------------------------------------------------------------------------------
def _family_d(b):
    names = list(TAGS)
    k = 0
    for ti, t in enumerate(names):
        for ii, ihl in enumerate((5, 6, 15)):
            # head frames of 42..182 bytes: shorter than a 64-byte window, between the two windows, past both; the
            # later fragments' tagging and header length differ from the head's (their payload is the frame's last
            # frag_len bytes, :248); the final's length and padding move the datagram's end over all four end & 3
            h, m, f, pad = (8, 40, 104)[(ti + ii) % 3], (8, 16, 24)[k % 3], 5 + k % 4, k % 3
            p = pat(h + m + f, 60 + k)
            hd = (17 if k % 2 else 6, 0, True, p[:h])
            md = (17, h, True, p[h:h + m])
            fn = (6, h + m, False, p[h + m:])
            kws = (dict(TAGS[t], ihl=ihl), dict(TAGS[names[(ti + 1) % 3]], ihl=(6, 15, 5)[ii]),
                   dict(TAGS[names[(ti + 2) % 3]], ihl=(15, 5, 6)[ii], pad=pad))
            order = ((0, 1, 2), (1, 2, 0), (1, 0, 2))[k % 3]      # in order; head last; head second (the scan, :337)
            c = b.case(f"D/{t}/ihl{ihl}", family="D")
            for n, q in enumerate(order):
                c.add(REASM if n == 2 else CACHED, *(hd, md, fn)[q], **kws[q])
            c.payload = p + bytes(pad)
            k += 1
    # a last segment inside one output dword, up to it, and one byte past it
    for n in (1, 2, 3):
        p = pat(8 + n, 80 + n)
        c = b.case(f"D/final_{n}_bytes", family="D")
        c.add(CACHED, 17, 0, True, p[:8]).add(REASM, 17, 8, False, p[8:])
        c.payload = p
    # ICMP with payload behind the head: the bytes the reference sized but never wrote (:257-265) read zero; a head
    # shorter than both windows, and one longer
    for name, h, f in (("short", 16, 24), ("long", 104, 30)):
        p = pat(h + f, 90 + h)
        b.case(f"D/icmp_fill_{name}", family="D").add(CACHED, 1, 0, True, p[:h]).add(REASM, 1, h, False, p[h:])


def cases():
    """Every case of the corpus, in a fixed order."""
    b = _Builder()
    _family_a(b)
    _family_b(b)
    _family_c(b)
    _family_d(b)
    return b.cases


def of_config(cs, cfg):
    return [c for c in cs if c.cfg == cfg]


def fcb_full_group(cs):
    """(cases, fcb_max, want per case): the `default` chains of families B and C that never complete (no FCB is freed
    by the aging calls between the batches of `columns`, so the running count only grows), under a table two FCBs
    short: fcb_create's cap (:75-82) fails the last two creators in index order, on their later fragments too (they
    find no FCB and try to create one again)."""
    g = [c for c in cs if c.cfg == "default" and c.family in "BC" and REASM not in c.want and DELETED not in c.want]
    want = [list(c.want) for c in g[:-2]] + [[FCB_FULL] * len(c.want) for c in g[-2:]]
    return g, len(g) - 2, want


def arena(frames, align=4):
    """(arena u8, off u64, len u32) of frames = [(bytes, wire length)]: frame starts on `align` bytes, the gaps (at
    least one byte behind every frame) and TAIL bytes behind the last filled with FILL."""
    assert align in (1, 4)
    off, buf = [], bytearray()
    for fr, _ in frames:
        off.append(len(buf))
        buf += fr
        buf += bytes([FILL]) * (1 if align == 1 else ((-len(buf)) % 4 or 4))
    buf += bytes([FILL]) * TAIL
    return (np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64),
            np.array([n for _, n in frames], np.uint32))


def arrangements(cs):
    """(name, batches) over the frames of cs; a batch is a list of (case index, frame index).
    together: one batch, the cases back to back.  interleaved: one batch, fragment k of every case in turn.  columns:
    batch k holds the k-th fragment of every case (Case.cols), so every chain crosses batches."""
    together = [(ci, fi) for ci, c in enumerate(cs) for fi in range(len(c.frames))]
    ncol = 1 + max(max(c.cols) for c in cs)
    cols = [[(ci, fi) for ci, c in enumerate(cs) for fi in range(len(c.frames)) if c.cols[fi] == k]
            for k in range(ncol)]
    yield "together", [together]
    yield "interleaved", [[x for col in cols for x in col]]
    yield "columns", cols


def layout(cs, batches, align=4, want=None):
    """One arena for a whole sequence, its frames in batch order: (arena, [(off, len, gid, want)] per batch).  gid: a
    frame's index in the `together` order, the same in every arrangement; want: the cases' own, or per case."""
    base = np.cumsum([0] + [len(c.frames) for c in cs])
    want = [c.want for c in cs] if want is None else want
    order = [x for bt in batches for x in bt]
    a, off, lens = arena([cs[ci].frames[fi] for ci, fi in order], align)
    out, at = [], 0
    for bt in batches:
        sl = slice(at, at + len(bt))
        out.append((off[sl], lens[sl], np.array([base[ci] + fi for ci, fi in bt], np.uint64),
                    np.array([want[ci][fi] for ci, fi in bt], np.uint32)))
        at += len(bt)
    return a, out
