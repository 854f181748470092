"""The attack monitors and the port-scan detector together on the flow-table path, as the reference runs them: Decode ->
DecodeIPV4 / DecodeTCP (monitors, decode-ipv4.c:141-149, decode-tcp.c:162-173) -> FlowHandlePacket -> FlowFind | miss ->
syn_check -> PortScan_Detect -> DP_Acl_Lookup -> FlowAdd with DP_Attack_SynCountMonitor (flow.c:120-158, :196-243), for the
tests of ppe_flow_combine.

Nothing new is modelled here.  Three existing parts are composed:
    AttackFlowModel.judge              (tests/attack_flow_model.py) decides, serially in index order, who is
                                       monitor-dropped; AttackFlowModel.classify_batch writes those rows and their
                                       counters as it does without the detector;
    FlowPortScanModel.classify_batch   (tests/flow_portscan_model.py) runs over the survivors in their order, with ts
                                       restricted to them: it takes the place of the oracle's flow table that
                                       AttackFlowModel hands its survivors to;
    syncount_accum                     +1 per survivor row with F_NEWFLOW | F_TCP | F_SYN on that packet's port, the
                                       line AttackFlowModel.classify_batch already has.
Neither model file is touched: FlowCombinedModel is an AttackFlowModel whose `ft` is the adapter below."""
import numpy as np

from attack_flow_model import AttackFlowModel
from attack_model import AttackModel
from flow_portscan_model import FlowPortScanModel


class _Survivors:
    """What AttackFlowModel calls its flow table: FlowPortScanModel over the packets handed to it, with their ts."""

    def __init__(self, fp: FlowPortScanModel):
        self.fp, self.ts, self.last = fp, None, None

    def classify_batch(self, hdr, lens, cfg=None):
        self.last = self.fp.classify_batch(hdr, lens, self.ts, cfg)
        return self.last

    def age(self, now, timeout=20):
        return self.fp.age(now, timeout)

    def close(self):
        pass


class FlowCombinedModel(AttackFlowModel):
    def __init__(self, oracle, atk: AttackModel, fp: FlowPortScanModel):
        self.o, self.atk, self.fp = oracle, atk, fp   # (no pyoracle.OracleFlow: the table is fp's)
        self.ft = _Survivors(fp)
        self._keep, self._ts = None, None

    def judge(self, hdr, lens, ports, cfg, punt=None):
        dec, drops = super().judge(hdr, lens, ports, cfg, punt)
        self._keep = np.array([i for i, d in enumerate(drops) if d is None], np.int64)
        self.ft.ts = None if self._ts is None else np.ascontiguousarray(self._ts, np.uint64)[self._keep]
        return dec, drops

    def classify_batch(self, hdr, lens, ports=None, ts=None, cfg=None):
        """One batch: AttackFlowModel.classify_batch's result (verdict, flow_hash, acl_hit, tuple, counters, dropped)
        and `results` (per packet PortScan_Detect's answer, -1 = not called: also every monitor drop)."""
        self._ts, self.ft.last = ts, None
        out = super().classify_batch(hdr, lens, ports, cfg)
        out["results"] = np.full(len(lens), -1, np.int64)
        if self.ft.last is not None:
            out["results"][self._keep] = self.ft.last["results"]
        return out

    def table(self):
        return self.fp.table()

    def stats(self):
        return self.fp.stats()
