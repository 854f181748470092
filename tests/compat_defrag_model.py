"""A serial model of a Decode flush with defrag_able == 1 (include/ppe_decode.h), composed from pyoracle.Oracle (the
stateless classify of a burst) and pyoracle.OracleDefrag (one core's Defrag), neither changed:

  1. the burst's frames are classified from their first 144 bytes;
  2. the frames with status FRAG go through Defrag in burst order (their ids are the caller's mbuf numbers);
  3. the datagrams they complete are classified from their whole frames as a second burst, in the order of their
     completing fragments;
  4. the hook calls, in burst order: a frame that is no fragment by its verdict (DP_Log_Func first on the logged
     drops); a cached fragment none; a fragment Defrag drops the drop hook (DP_Log_Func first when the cache is full);
     a completing fragment its datagram's one call.

An event is (hook, who): hook "fw" / "drop" / "punt" / "log", who an mbuf number or ("dgram", mbuf number of the
completing fragment).  The model keeps each datagram's frame, chain (mbuf numbers in chain order) and verdict in
`dgrams`.  tests/test_compat_defrag_model.py pins it with hand-derived sequences."""
import numpy as np

import pyoracle
from ppe import abi
from ppe.abi import ST

W = 144   # Decode's header window (PPE_COMPAT_STRIDE)
LOGGED = {ST[k] for k in ("L2_HEADER_ERR", "VLAN_HEADER_ERR", "IPV4_HEADER_ERR", "IPV4_VERSION_ERR", "IPV4_LEN_ERR",
                          "FRAG_LEN_ERR", "UDP_HEADER_ERR", "UDP_LEN_ERR", "TCP_HEADER_ERR", "TCP_LEN_ERR",
                          "ACL_DROP")}
HOOKS = {0: "fw", 1: "drop", 2: "punt"}   # PPE_ACT_FW / _DROP / _PUNT (include/ppe_hip.h)
DF = abi.DF


def windows(frames):
    hdr = np.zeros((len(frames), W), np.uint8)
    lens = np.zeros(len(frames), np.uint32)
    for i, f in enumerate(frames):
        c = min(len(f), W)
        hdr[i, :c] = np.frombuffer(bytes(f[:c]), np.uint8)
        lens[i] = len(f)
    return hdr, lens


class DecodeDefragModel:
    def __init__(self, rules, default_action=1, cache_max=8):
        self.o = pyoracle.Oracle(rules, default_action=default_action)
        self.d = pyoracle.OracleDefrag(fcb_max=1024, cache_max=cache_max)
        self.dgrams = {}      # mbuf number of the completing fragment -> dict(frame, chain, verdict, hit)
        self.verdict = {}     # mbuf number -> the first classify's verdict
        self.status = {}      # mbuf number of a fragment -> its Defrag status word

    def close(self):
        self.d.close()

    def _by_verdict(self, events, who, v):
        st, act = int(v) & 0xFF, (int(v) >> 8) & 0xFF
        if act == 1 and st in LOGGED:
            events.append(("log", who))
        events.append((HOOKS.get(act, "punt"), who))

    def flush(self, frames, ids, now, defrag_able=1):
        """frames: the burst's whole frames (bytes); ids: their mbuf numbers.  Returns the events in order."""
        hdr, lens = windows(frames)
        v = self.o.classify_batch(hdr, lens, cfg=self.o.cfg(0, 1, 0))["verdict"]
        for i, m in enumerate(ids):
            self.verdict[m] = int(v[i])
        fr = [i for i in range(len(frames)) if (int(v[i]) & 0xFF) == ST["FRAG"]] if defrag_able == 1 else []
        disp = {}
        if fr:
            buf, off = bytearray(), []
            for i in fr:
                off.append(len(buf))
                buf += frames[i]
                buf += bytes((-len(buf)) % 4)
            buf += bytes(64)
            ref = self.d.batch(np.frombuffer(bytes(buf), np.uint8), np.array(off, np.uint64),
                               np.array([len(frames[i]) for i in fr], np.uint32), now,
                               ids=np.array([ids[i] for i in fr], np.uint64))
            nd = ref["n_dgram"]
            dfr = [bytes(ref["dgram_pkt"][j, :int(ref["dgram_len"][j])]) for j in range(nd)]
            if nd:
                dh, dl = windows(dfr)
                r2 = self.o.classify_batch(dh, dl, cfg=self.o.cfg(0, 1, 0))
            for k, i in enumerate(fr):
                st = int(ref["status"][k])
                self.status[ids[i]] = st
                disp[i] = st & 0xFF
                if st & 0xFF == DF["REASM"]:
                    j = int(ref["dgram_of"][k])
                    self.dgrams[ids[i]] = dict(frame=dfr[j], verdict=int(r2["verdict"][j]), hit=int(r2["acl_hit"][j]),
                                               chain=[int(x) for x in ref["dgram_frags"][j] if int(x) != 2**64 - 1])
        events = []
        for i, m in enumerate(ids):
            s = disp.get(i)
            if s is None or s == DF["NOT_FRAG"]:
                self._by_verdict(events, m, v[i])
            elif s in (DF["CACHED"], DF["SETUP_ERR"]):
                pass
            elif s == DF["REASM"]:
                self._by_verdict(events, ("dgram", m), self.dgrams[m]["verdict"])
            else:
                if s == DF["CACHE_FULL"]:
                    events.append(("log", m))
                events.append(("drop", m))
        return events

    def age(self, now):
        """DP_Defrag_Age: the drop-hook calls (in no particular order: compare sorted)."""
        ids, _ = self.d.age(now, 20)
        return sorted(("drop", int(x)) for x in ids)
