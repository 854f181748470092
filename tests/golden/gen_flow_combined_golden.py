"""Writes tests/golden/flow_combined_v1.npz: one generated scenario of tests/flow_combined_model.py (the attack monitors
ahead of FlowGetFlowFromHash with PortScan_Detect inside; ticks and aging between the batches) frozen as model output
only, so that a change of the composition, of the generator or of the models under it shows
(tests/test_flow_combined_model.py replays it on the CPU, tests/test_gpu_flow_combined.py on the GPU).

Run from the repository root after the build: python tests/golden/gen_flow_combined_golden.py"""
import sys
from collections import Counter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle")]

from test_flow_combined_model import gen_combined, run_generated, state_rows  # noqa: E402

SEED, BATCHES, MAX_N = 91, 12, 96

if __name__ == "__main__":
    seq, par = gen_combined(SEED, BATCHES, MAX_N)
    ev = Counter()
    outs, m = run_generated(seq, par, ev=ev)
    np.savez_compressed(Path(__file__).resolve().parent / "flow_combined_v1.npz", seed=SEED, batches=BATCHES, max_n=MAX_N,
                        verdict=np.concatenate([o["verdict"] for o in outs]),
                        flow_hash=np.concatenate([o["flow_hash"] for o in outs]),
                        acl_hit=np.concatenate([o["acl_hit"] for o in outs]),
                        results=np.concatenate([o["results"] for o in outs]),
                        counters=sum(o["counters"] for o in outs),
                        flows=np.array(m.table(), np.uint64).reshape(-1, 10),
                        records=np.array(sorted(m.fp.ps.records()), np.uint64).reshape(-1, 7),
                        attack=state_rows(m))
    print("packets", sum(len(s["lens"]) for s in seq), "events", dict(ev), "flows", len(m.fp.flows))
