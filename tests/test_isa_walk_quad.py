"""The probe loop's quad protocol in the static instruction stream
(tools/isa_check.py, CPU: needs only hipcc).

A probe's owner lane sits in the quad that reads its bucket, and the bucket
index, the parent and the word reach the quad by DPP moves: nothing of the
request goes through LDS, and no LDS read stands between the loop head's pop
and the bucket loads.  The found slot goes back with one ds_write_b128.

Measured on the tree this test came with, production instantiation
tm_match_tiles<false, false, 384>: the copy that reads the topic's words from
LDS holds 322 static instructions (189 VALU, 15 LDS, 8 VMEM, 53 exec-mask SALU,
13 branches, 29 other SALU, 13 waits, 2 s_nop, 0 lane moves), the copy that
reads them from HBM 328 (13 LDS).  The ceiling is 5 % above the 322: 338.
The 15 LDS operations: the pop, the topic's offset and depth (one read), two
words, the tail words (two paired writes), four slot writes, the result, the
row count, two pushes and the row-count atomic.
"""

import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MEASURED = 322
CEILING = 338     # MEASURED * 1.05, rounded down
LDS_OPS = 15      # LDS-words copy, measured

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not shutil.which("hipcc"),
                                reason="needs hipcc")


@pytest.fixture(scope="module")
def listing():
    import isa_check
    return isa_check.walk_asm()


@pytest.fixture(scope="module")
def production(listing):
    import isa_check
    rep = isa_check.walk_report(listing)
    assert isa_check.PRODUCTION_WALK in rep, sorted(rep)
    return rep[isa_check.PRODUCTION_WALK]


def loop_bodies(listing):
    """The instruction rows [(op, args)] of the production kernel's probe loops,
    found as isa_check.probe_loops finds them: innermost label-to-backward-branch
    spans that hold the bucket loads."""
    import isa_check
    m = re.search(r"^%s:" % re.escape(isa_check.PRODUCTION_WALK), listing, re.M)
    body = listing[m.end():listing.find(".Lfunc_end", m.end())]
    rows = isa_check._instrs(body)
    at = {lab: i for i, (lab, _, _) in enumerate(rows) if lab}
    spans = {}
    for i, (_, op, args) in enumerate(rows):
        if op and op.startswith(("s_cbranch", "s_branch")) and at.get(args.strip(), i) < i:
            b = at[args.strip()]
            spans[b] = max(spans.get(b, 0), i)
    loads = [i for i, (_, op, _) in enumerate(rows) if op == "buffer_load_dwordx4"]
    found = []
    for b, e in sorted(spans.items(), key=lambda s: s[1] - s[0]):
        if any(b <= i <= e for i in loads) and not any(b2 <= b and e <= e2 or b <= b2 and e2 <= e for b2, e2 in found):
            found.append((b, e))
    return [[(op, args) for _, op, args in rows[b:e + 1] if op] for b, e in sorted(found)]


def test_the_request_does_not_go_through_lds(listing, production):
    """Between a loop's head and its first bucket load there is the pop (one
    ds_read_b128) and no other LDS operation: no ds_read_b32 of a bucket index,
    no write of one."""
    bodies = loop_bodies(listing)
    assert len(bodies) == len(production["loops"]) == 2
    for body in bodies:
        ops = [op for op, _ in body]
        head = ops[:ops.index("buffer_load_dwordx4")]
        assert "ds_read_b32" not in head, head
        assert [op for op in head if op.startswith("ds_")] == ["ds_read_b128"], head
        # the quad takes the request by DPP: a quad_perm broadcast feeds every load's offset
        dpp = [args for op, args in body if op.endswith("_dpp") and "quad_perm" in args]
        for r in range(4):
            assert any("quad_perm:[%d,%d,%d,%d]" % (r, r, r, r) in a for a in dpp), (r, dpp)
        assert ops.count("ds_write_b128") >= 4      # four whole-slot reports (and the pushes)


def test_lds_operations_of_the_loop(production):
    for lp in production["loops"]:
        assert lp["bucket_loads"] == 4 and lp["lane"] == 0, lp
    lds = [lp for lp in production["loops"] if lp["words"] == "lds"]
    assert len(lds) == 1
    assert lds[0]["lds"] <= LDS_OPS, lds[0]
    hbm = [lp for lp in production["loops"] if lp["words"] == "hbm"]
    assert len(hbm) == 1 and hbm[0]["lds"] <= LDS_OPS - 2, hbm[0]     # its two word reads are global loads


def test_probe_loop_stays_under_the_ceiling(production):
    assert CEILING == MEASURED * 105 // 100
    lds = [lp for lp in production["loops"] if lp["words"] == "lds"]
    assert lds[0]["total"] <= CEILING, lds[0]


def test_resource_envelope(production):
    """Four waves per SIMD: at most 128 VGPRs, the 384-entry stack's 9,216 B of LDS, no scratch."""
    assert production["vgpr"] <= 128 and production["vgpr_spill"] == 0
    assert production["lds"] == 9216 and production["scratch"] == 0
