"""The port-scan detector and the TCP sessions on one flow batch (ppe_flow_stream_portscan), without the attack monitors
(launch kind 7) and with them (kind 8), as the reference runs its default pipeline: Decode -> attack monitors ->
FlowHandlePacket -> FlowFind | miss -> syn_check -> PortScan_Detect -> DP_Acl_Lookup -> FlowAdd (syncount_accum) ->
FlowUpdate -> StreamTcp (flow.c:196-243, :271-320).

A composition, nothing re-modelled and no model file edited:
    rows and tables    tests/flow_portscan_model.py's FlowPortScanModel (kind 7), or tests/flow_combined_model.py's
                       FlowCombinedModel over it (kind 8: the monitors first, the survivors to the detector's path, +1 of
                       syncount_accum per SYN-created flow);
    sessions           tests/flow_stream_attack_model.py's FlowStreamAttackModel.classify_batch, unchanged: every packet
                       that ends ACL_FW with F_FLOW | F_TCP steps tests/stream_session_model.py's machine in index order,
                       a F_NEWFLOW packet from the zero record; the before / after rule gives syncount_accum its -1 on the
                       completing packet's port; the creating packet's port is the flow's; aging releases.
StreamTcp's verdict feeds nothing back (an ERR is output_drop_proc behind FlowAdd and FlowUpdate, flow.c:304-319): the
session pass runs over the finished rows of the batch and changes verdict words and OUT_FW / OUT_DROP only.  A packet
with status 24, NO_SYN, ACL_DROP or FLOW_NOMEM has no F_FLOW: it takes no step and counts in no stream counter.
Kind 7 has no monitors: its accumulators are a stub nobody reads and every flow's port is 0."""
import numpy as np

import stream_session_model as m
from flow_combined_model import FlowCombinedModel
from flow_stream_attack_model import FlowStreamAttackModel, ends


class _NoMonitors:
    """Kind 7: what FlowStreamAttackModel adds its -1 to when no monitors exist."""

    def __init__(self):
        self.ai = [dict(syncount_accum=0) for _ in range(4)]


class _Rows:
    """What FlowStreamAttackModel calls its AttackFlowModel: the detector's model, alone or behind the monitors."""

    def __init__(self, inner, combined):
        self.inner, self.combined, self.ts = inner, combined, None

    def classify_batch(self, hdr, lens, ports, cfg=None):
        if self.combined:
            return self.inner.classify_batch(hdr, lens, ports, self.ts, cfg)
        return self.inner.classify_batch(hdr, lens, self.ts, cfg)

    def close(self):
        pass


class FlowStreamPortScanModel(FlowStreamAttackModel):
    def __init__(self, oracle, fp, atk=None, track=1):
        """fp: a FlowPortScanModel (its PortScanModel's able decides whether the detector runs); atk: an AttackModel
        for kind 8, None for kind 7; track 0: the rows alone, no session is stepped."""
        self.o, self.fp, self.track = oracle, fp, track
        self.kind = 8 if atk is not None else 7
        self.rows = FlowCombinedModel(oracle, atk, fp) if atk is not None else fp
        self.afm = _Rows(self.rows, atk is not None)
        self.ft = fp  # (age())
        self.atk = atk if atk is not None else _NoMonitors()
        self.ssn, self.port, self.cnt = {}, {}, m.Counters()

    def classify_batch(self, hdr, lens, ports=None, ts=None, cfg=None):
        """One batch: the rows' result (verdict, flow_hash, acl_hit, tuple, counters, results) with the sessions'
        verdicts, and the reasons per packet."""
        self.afm.ts = ts
        if self.kind == 7:
            ports = None
        if not self.track:
            return self.afm.classify_batch(hdr, lens, ports, cfg), np.zeros(len(lens), np.uint32)
        return super().classify_batch(hdr, lens, ports, cfg)

    def tcp_keys(self):
        return {ends(f["sip"], f["dip"], f["sport"], f["dport"]) for f in self.fp.flows.values() if f["protocol"] == 6}

    def age(self, now, timeout=20, release=True):
        return super().age(now, timeout, release and self.kind == 8)

    def table(self):
        return self.fp.table()

    def stats(self):
        return self.fp.stats()
