"""Per-kernel ISA census of tm_kernels.hip (dev tool): instruction count,
scratch and flat memory ops -- a kernel-argument array indexed at run time is
copied to scratch and every pointer it reaches becomes flat (slow).

    python tools/isa_check.py [kernel-substring]
    python tools/isa_check.py --walk [listing.s]   # the walk kernels' registers, spills and probe-loop mix
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hipcc() -> str:
    """The compiler the test's skip check found: /opt/rocm/bin/hipcc, else hipcc on PATH."""
    import shutil
    if os.path.exists("/opt/rocm/bin/hipcc"):
        return "/opt/rocm/bin/hipcc"
    return shutil.which("hipcc") or "hipcc"


def census():
    """{kernel symbol: (instructions, scratch ops, flat ops)} of the gfx950 build."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(ROOT, "emqx_amd", "csrc", "tm_kernels.hip"), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        s = open(out).read()
    res = {}
    for m in re.finditer(r"^(_ZN3etm\w+):", s, re.M):
        name = m.group(1)
        j = s.find(".Lfunc_end", m.end())
        body = s[m.end():j]
        ops = [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and ln.split() and not ln.startswith("\t.")]
        c = collections.Counter(ops)
        scratch = sum(v for k, v in c.items() if k.startswith("scratch_"))
        flat = sum(v for k, v in c.items() if k.startswith("flat_"))
        res[name] = (len(ops), scratch, flat)
    return res


def walk_asm(defines=()):
    """The gfx950 assembly listing of tm_kernels.hip (text)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", *defines,
                        os.path.join(ROOT, "emqx_amd", "csrc", "tm_kernels.hip"), "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


# Static instruction classes of the walk's probe loop.  "lane" is v_readlane /
# v_writelane: in this loop every one of them moves a spilled SGPR (the loop's
# own code uses no readlane builtin).  "exec" is the SALU that builds, saves and
# restores lane masks: any *_saveexec, any operand named exec, and the 64-bit
# logic ops that combine compare results.
CLASSES = ("valu", "lds", "vmem", "exec", "branch", "salu", "wait", "nop", "lane")
_MASK_OPS = re.compile(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor|not|cselect)_b64$")


def classify(op, args=""):
    if op in ("v_readlane_b32", "v_writelane_b32"):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_nop":
        return "nop"
    if "saveexec" in op or re.search(r"\bexec(_lo|_hi)?\b", args) or _MASK_OPS.match(op):
        return "exec"
    return "salu"


def _instrs(body):
    """[(label or None, op, args)] of a kernel body, labels as their own rows."""
    rows = []
    for ln in body.split("\n"):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            rows.append((m.group(1), None, ""))
        elif ln.startswith("\t") and not ln.startswith("\t.") and not ln.lstrip().startswith(";") and ln.split():
            parts = ln.split(None, 1)
            rows.append((None, parts[0], parts[1].split(";")[0] if len(parts) > 1 else ""))
    return rows


def probe_loops(body):
    """The innermost loops of a kernel body that hold the bucket loads
    (buffer_load_dwordx4): a loop is the span from a label to the last backward
    branch to it.  -> [{class: count, ..., "total", "bucket_loads", "words"}],
    "words" being "lds" or "hbm" (the copy that reads the topic's words with
    global loads)."""
    rows = _instrs(body)
    at = {lab: i for i, (lab, _, _) in enumerate(rows) if lab}
    spans = {}
    for i, (_, op, args) in enumerate(rows):
        if op and op.startswith(("s_cbranch", "s_branch")):
            tgt = args.strip()
            if tgt in at and at[tgt] < i:
                spans[at[tgt]] = max(spans.get(at[tgt], 0), i)
    loads = [i for i, (_, op, _) in enumerate(rows) if op == "buffer_load_dwordx4"]
    found = []
    for b, e in sorted(spans.items(), key=lambda s: s[1] - s[0]):
        mine = [i for i in loads if b <= i <= e]
        if not mine or any(b2 <= b and e <= e2 for b2, e2 in found):
            continue
        if any(b <= b2 and e2 <= e for b2, e2 in found):
            continue   # an outer loop of one already found
        found.append((b, e))
    res = []
    for b, e in sorted(found):
        c = collections.Counter(classify(op, args) for _, op, args in rows[b:e + 1] if op)
        mix = {k: c.get(k, 0) for k in CLASSES}
        mix["total"] = sum(c.values())
        mix["bucket_loads"] = sum(1 for i in loads if b <= i <= e)
        mix["words"] = "hbm" if any(op == "global_load_dword" for _, op, _ in rows[b:e + 1]) else "lds"
        res.append(mix)
    return res


def walk_report(asm=None):
    """{walk kernel symbol: {"sgpr_spill", "vgpr_spill", "vgpr", "sgpr", "lds", "scratch", "lane_moves", "loops"}}
    from the listing's kernel metadata and bodies."""
    s = asm if asm is not None else walk_asm()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", s[s.find("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "tm_match_tiles" not in name.group(1):
            continue
        def num(key):
            m = re.search(r"\." + key + r":\s+(\d+)", blk)
            return int(m.group(1)) if m else 0
        meta[name.group(1)] = {"sgpr_spill": num("sgpr_spill_count"), "vgpr_spill": num("vgpr_spill_count"),
                               "vgpr": num("vgpr_count"), "sgpr": num("sgpr_count"),
                               "lds": num("group_segment_fixed_size"), "scratch": num("private_segment_fixed_size")}
    for m in re.finditer(r"^(_ZN3etm14tm_match_tiles\w+):", s, re.M):
        name = m.group(1)
        body = s[m.end():s.find(".Lfunc_end", m.end())]
        ops = [op for _, op, _ in _instrs(body) if op]
        meta.setdefault(name, {})
        meta[name]["lane_moves"] = sum(1 for op in ops if classify(op) == "lane")
        meta[name]["loops"] = probe_loops(body)
    return meta


PRODUCTION_WALK = "_ZN3etm14tm_match_tilesILb0ELb0ELi384EEEvNS_9MatchArgsE"


def print_walk_report(rep):
    for name, r in rep.items():
        print(f"{name}\n  sgpr_spill {r['sgpr_spill']} vgpr_spill {r['vgpr_spill']} vgpr {r['vgpr']} sgpr {r['sgpr']} "
              f"lds {r['lds']} B scratch {r['scratch']} B  readlane/writelane kernel-wide {r['lane_moves']}")
        for lp in r["loops"]:
            print(f"  probe loop ({lp['words']} words): {lp['total']} static instrs, bucket loads {lp['bucket_loads']}: "
                  + " ".join(f"{k} {lp[k]}" for k in CLASSES))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--walk":   # python tools/isa_check.py --walk [listing.s]
        asm = open(sys.argv[2]).read() if len(sys.argv) > 2 else None
        print_walk_report(walk_report(asm))
        return 0
    want = sys.argv[1] if len(sys.argv) > 1 else ""
    bad = 0
    for name, (n, scratch, flat) in census().items():
        if want in name:
            print(f"{name[:70]:70s} instrs {n:6d} scratch {scratch:4d} flat {flat:4d}")
        bad += scratch + flat
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
