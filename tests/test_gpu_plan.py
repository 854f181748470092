"""The engine's cached launch plans cannot go stale: after every event that changes the image or the tuning (commit,
tuning change, stage without publish, publish, a flow-table launch in between) ppe_launch_info reports what the
planner computes for the running image and the current tuning, and the launch gives the oracle's results.

Batches of 4,097 packets: 65 tiles, a partial last tile and a partial multi-tile round.  Reference: the oracle's
linear classify_batch (bit-exact integer work, no tolerance), with the 64-B window's rule for the few packets whose
headers reach past it (assert_same)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402

NOW = 1_700_000_000
DEV = torch.device("cuda:0")
N = 4097
KEYS = ("verdict", "flow_hash", "acl_hit")
FETCH = {0: "none", 1: "hoist", 3: "multi", 5: "cut"}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


class Traffic:
    """One packet batch on the device, with room for its results."""

    def __init__(self, rules, seed):
        self.pk = synth.make_packets(N, rules, seed=seed, kind="imix", stride=64)
        self.hdr = torch.from_numpy(self.pk["hdr"]).to(DEV)
        self.len = torch.from_numpy(self.pk["len"].view(np.int32)).to(DEV)

    def out(self):
        return {k: torch.full((N,), -7, dtype=torch.int32, device=DEV) for k in KEYS}

    def classify(self, eng):
        out = self.out()
        eng.classify_torch(self.hdr, self.len, out, cfg=eng.cfg(now_seconds=NOW))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().view(np.int32 if k == "acl_hit" else np.uint32) for k, v in out.items()}

    def oracle(self, rules):
        o = pyoracle.Oracle(rules, default_action=1)
        return o.classify_batch(self.pk["hdr"], self.pk["len"], cfg=o.cfg(now_seconds=NOW))


def same(got, ref):
    return all(np.array_equal(got[k], ref[k]) for k in KEYS)


def assert_same(got, ref, what):
    """Bit-exact, but for the packets whose headers reach past the 64-B window (the oracle's reach > 64: malformed
    ones with IPv4 options), which the engine punts as WINDOW_PUNT whatever the oracle finds behind the window."""
    far = ref["reach"] > 64 if "reach" in ref else np.zeros(N, bool)
    for k in KEYS:
        bad = np.flatnonzero((got[k] != ref[k]) & ~far)
        assert not len(bad), f"{what}: {k}: {len(bad)} mismatches, first {bad[:5].tolist()}"
    assert ((got["verdict"][far] & 0xFFFF) == (abi.ST["WINDOW_PUNT"] | abi.ACT_PUNT << 8)).all(), what


def assert_plan_is_current(eng, what):
    """ppe_launch_info (the cached stateless plan of the running slot) == the planner on the running image and the
    current tuning; returns the plan."""
    img = eng.image()
    t, p = abi.Tuning(**eng.tuning()), abi.Plan()
    assert eng.lib.ppe_plan_image(img.ctypes.data, len(img), C.byref(t), 0, C.byref(p)) == 0
    info = eng.launch_info()
    want = {"block": p.block, "lds_bytes": p.lds_bytes, "image": ("global", "lds", "split")[p.mode],
            "fetch": FETCH[p.pipe]}
    assert {k: info[k] for k in want} == want, what
    return p.as_dict()


def check(eng, traffic, ref, what):
    plan = assert_plan_is_current(eng, what)
    assert_same(traffic.classify(eng), ref, what)
    return plan


def test_cached_plans_follow_image_and_tuning(eng):
    rules_a, rules_b = synth.make_rules(256, seed=256), synth.make_rules(1024, seed=1024)
    rules_c = synth.make_rules(256, seed=77)
    base = eng.tuning()
    try:
        # 1. 256 rules (the tree fits in LDS): every tuning change replans
        eng.commit(rules_a, default_action=1)
        ta = Traffic(rules_a, 5)
        ref_a = ta.oracle(rules_a)
        seen = set()
        for tune in (dict(), dict(lds_image=0), dict(block=1024), dict(pipeline=1), dict(pipeline=3)):
            eng.tuning(**{**base, **tune})
            p = check(eng, ta, ref_a, f"256 rules, {tune}")
            seen.add((p["mode"], p["pipe"], p["block"]))
        assert len(seen) == 5  # (five different kernel variants: a stale plan would repeat one)
        eng.tuning(**base)
        check(eng, ta, ref_a, "256 rules, tuning restored")

        # 2. 1,024 rules: the running slot flips, the default plan is the cut lists
        eng.commit(rules_b, default_action=1)
        tb = Traffic(rules_b, 6)
        ref_b = tb.oracle(rules_b)
        p = check(eng, tb, ref_b, "1024 rules, default tuning")
        assert FETCH[p["pipe"]] == "cut"
        eng.tuning(**{**base, "pipeline": 3})
        p = check(eng, tb, ref_b, "1024 rules, pipeline 3")
        assert FETCH[p["pipe"]] == "multi"
        eng.tuning(**base)

        # 3. a staged, unpublished image changes nothing; publishing it does
        tc = Traffic(rules_c, 7)
        ref_cb, ref_cc = tc.oracle(rules_b), tc.oracle(rules_c)
        assert not same(ref_cb, ref_cc)  # (the two rule sets classify this batch differently)
        info_b = eng.launch_info()
        token, _ = eng.stage(rules_c, default_action=1)
        assert eng.launch_info() == info_b
        check(eng, tc, ref_cb, "1024 rules running, 256 staged")
        eng.publish(token)
        p = check(eng, tc, ref_cc, "256 rules published")
        assert eng.launch_info() != info_b and FETCH[p["pipe"]] == "hoist"

        # 4. a flow-table launch (the slot's other plan) in between leaves the stateless plan as it was
        before = tc.classify(eng)
        eng.flow_create(10_000, 8192)
        try:
            eng.classify_flow_torch(tc.hdr, tc.len, tc.out(), cfg=eng.cfg(now_seconds=NOW))
            torch.cuda.synchronize()
            assert_plan_is_current(eng, "after a flow-table launch")
            assert_same(tc.classify(eng), before, "stateless after a flow-table launch")
        finally:
            eng.flow_destroy()
    finally:
        eng.tuning(**base)
