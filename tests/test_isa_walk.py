"""The static instruction stream of the walk's probe loop (tools/isa_check.py
walk_report, CPU: needs only hipcc).

The frontier loop of tm_match_tiles is bound by the instructions a wave issues
per iteration, and it once grew from 406 to 522 static
instructions, a quarter of them exec-mask bookkeeping and SGPR-spill lane
moves, without anyone noticing.  This test is the notice.

Measured on the tree this test came with, production instantiation
tm_match_tiles<false, false, 384>: the copy that reads the topic's words from
LDS holds 388 static instructions (222 VALU, 24 LDS, 8 VMEM, 57 exec-mask SALU,
17 branches, 35 other SALU, 16 waits, 9 s_nop, 0 lane moves), the copy that
reads them from HBM 393.  The ceiling is 5 % above the 388: 407.
"""

import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MEASURED = 388
CEILING = 407     # MEASURED * 1.05, rounded down

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not shutil.which("hipcc"),
                                reason="needs hipcc")


@pytest.fixture(scope="module")
def production():
    import isa_check
    rep = isa_check.walk_report()
    assert isa_check.PRODUCTION_WALK in rep, sorted(rep)
    return rep[isa_check.PRODUCTION_WALK]


def test_probe_loops_hold_four_bucket_loads_and_no_spill_moves(production):
    loops = production["loops"]
    assert sorted(lp["words"] for lp in loops) == ["hbm", "lds"], loops
    for lp in loops:
        assert lp["bucket_loads"] == 4, lp
        assert lp["lane"] == 0, lp      # v_readlane / v_writelane: a spilled SGPR read back every iteration


def test_probe_loop_stays_under_the_ceiling(production):
    assert CEILING == MEASURED * 105 // 100
    lds = [lp for lp in production["loops"] if lp["words"] == "lds"]
    assert len(lds) == 1
    assert lds[0]["total"] <= CEILING, lds[0]


def test_resource_envelope(production):
    """Four waves per SIMD: at most 128 VGPRs, the 384-entry stack's 9,216 B of LDS, no scratch."""
    assert production["vgpr"] <= 128 and production["vgpr_spill"] == 0
    assert production["lds"] == 9216 and production["scratch"] == 0
