"""Per-subscriber inboxes (tm_batch_inboxes), the parts that need no device:
the host restatement of the `SubPid ! {deliver, To, Msg}` loop
(emqx_broker.mailboxes) against hand-derived mailboxes and against the oracle's
Broker, the ABI's argument checks, and the NIF's terms.  The device paths are
in test_gpu_inbox.py."""

import ctypes as C
import os
import random
import shutil
import subprocess

import pytest
from conftest import lb, load_golden

from emqx_amd import _native as N
from emqx_amd import emqx_broker as B
from emqx_amd.engine import Engine
from oracle import oracle as O

DIRTY_IO = 2


def test_mailboxes_known_answers():
    kat = load_golden("kat_inbox.json")
    assert len(kat["cases"]) >= 3
    for case in kat["cases"]:
        rows = [[(lb(to), pid) for to, pid in row] for row in case["rows"]]
        want = {pid: [(i, lb(to)) for i, to in box] for pid, box in case["mailboxes"].items()}
        assert B.mailboxes(rows) == want, case["name"]


def test_mailboxes_against_the_oracle_broker():
    rng = random.Random(21)
    words = [b"a", b"b", b"c", b"+", b"#"]
    filters = set()
    while len(filters) < 60:
        ws = [rng.choice(words) for _ in range(rng.randint(1, 4))]
        if b"#" not in ws[:-1]:
            filters.add(b"/".join(ws))
    filters = sorted(filters)
    orc = O.Broker()
    for _ in range(400):
        orc.subscribe(rng.choice(filters), rng.randrange(40))
    topics = [b"/".join(rng.choice([b"a", b"b", b"c", b"d"]) for _ in range(rng.randint(1, 4))) for _ in range(300)]
    rows = [orc.publish(t) for t in topics]
    boxes = B.mailboxes(rows)
    # every delivery is in exactly one mailbox, and a mailbox is its pid's
    # subsequence of the dispatch order: publishes ascending, within a publish
    # the row's order
    assert sum(len(v) for v in boxes.values()) == sum(len(r) for r in rows)
    for pid, box in boxes.items():
        want = [(i, to) for i, row in enumerate(rows) for to, p in row if p == pid]
        assert box == want and want, pid
    assert set(boxes) == {p for row in rows for _, p in row}


def _last_error(L) -> str:
    return (L.tm_last_error() or b"").decode()


def test_abi_validation_host_only():
    """Every TM_EINVAL of tm_batch_inboxes that needs no device, and TM_ENODEV
    (a host-only engine's batch never runs: 'not waited' and the
    TM_BATCH_DEDUP refusal are in test_gpu_inbox.py)."""
    eng = Engine(device=-1)
    L = eng.L
    out = N.Inboxes()
    assert L.tm_inbox_tile() == 4096
    assert L.tm_batch_inboxes(None, None, 0, C.byref(out)) == N.TM_EINVAL
    assert L.tm_batch_inboxes(eng.h, None, 0, None) == N.TM_EINVAL and "out is NULL" in _last_error(L)
    assert L.tm_batch_inboxes(eng.h, None, 2, C.byref(out)) == N.TM_EINVAL and "unknown flag" in _last_error(L)
    assert L.tm_batch_inboxes(eng.h, None, N.TM_INBOX_DEVICE | 8, C.byref(out)) == N.TM_EINVAL
    assert L.tm_batch_inboxes(eng.h, None, 0, C.byref(out)) == N.TM_ENODEV
    assert L.tm_batch_inboxes(eng.h, None, N.TM_INBOX_DEVICE, C.byref(out)) == N.TM_ENODEV
    b = eng.prepare([b"a"])
    for call in (b.inboxes, b.inboxes_device):
        with pytest.raises(N.TmError) as ei:
            call()
        assert ei.value.rc == N.TM_ENODEV
    b.free()
    eng.close()


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_ctypes_mirror_matches_the_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(tm_inboxes));', 'printf("TM_INBOX_DEVICE %u\\n", (unsigned)TM_INBOX_DEVICE);']
    for f in N.Inboxes._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(tm_inboxes, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(N.Inboxes) and int(got["TM_INBOX_DEVICE"]) == N.TM_INBOX_DEVICE
    for f in N.Inboxes._fields_:
        assert int(got[f[0]]) == getattr(N.Inboxes, f[0]).offset, f[0]


def test_nif_deliver_batch_terms():
    from nif_harness import Nif
    nif = Nif()
    assert nif.flags("deliver_batch", 2) == DIRTY_IO
    e = nif.new(-1)
    assert nif.call("subscribe", e, b"a/+", 3, 0) == "ok"
    for bad in [("deliver_batch", e, ["a"]), ("deliver_batch", e, [b"a", 3]), ("deliver_batch", e, b"a"),
                ("deliver_batch", b"e", [b"a"])]:
        assert nif.call(*bad) == ("#badarg",), bad[2:]
    assert nif.call("deliver_batch", e, [b"a/b"]) == ("error", "enodev")
    assert nif.call("deliver_batch", e, []) == ("error", "enodev")
    nif.drop(e)
