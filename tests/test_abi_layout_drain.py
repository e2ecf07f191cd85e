"""The C ABI of the session drain without a device: the new ctypes mirrors and
constants against include/emqx_tm.h by a compiled sizeof / offsetof program."""

import ctypes as C
import os
import shutil
import subprocess

import pytest

from emqx_amd import _native as N
from emqx_amd import emqx_session as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [("tm_drain_session", N.DrainSession), ("tm_drain_in", N.DrainIn), ("tm_drain_record", N.DrainRecord),
         ("tm_drain_out", N.DrainOut)]
CONSTS = ["TM_QMSG_EXPIRY", "TM_QMSG_CLASS_SHIFT", "TM_DRAIN_BATCH_N", "TM_DRAIN_NO_ORDER", "TM_DRAIN_SEND0",
          "TM_DRAIN_SEND", "TM_DRAIN_KEPT", "TM_DRAIN_EXPIRED", "TM_DRAIN_COUNT", "TM_SESS_UNBOUNDED"]


@pytest.mark.skipif(not shutil.which("gcc"), reason="needs gcc")
def test_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "emqx_tm.h"', "int main(void) {"]
    for cname, py in PAIRS:
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    for c in CONSTS:
        lines.append(f'printf("const {c} %llu\\n", (unsigned long long){c});')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        k1, k2, v = ln.split()
        got[(k1, k2)] = int(v)
    for cname, py in PAIRS:
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])
    for c in CONSTS:
        assert got[("const", c)] == getattr(N, c), c
        if hasattr(S, c):
            assert got[("const", c)] == getattr(S, c), c
    assert C.sizeof(N.DrainSession) == 8 and C.sizeof(N.DrainRecord) == 16
    assert C.sizeof(N.DrainIn) == 56 and C.sizeof(N.DrainOut) == 88
