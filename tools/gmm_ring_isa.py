#!/usr/bin/env python3
"""The record-ring loop of K1 (csrc/gmm_outprob.hip, gmm_tile_ring_kernel) as the compiler emitted it, and the rule the
kernel's comment states, checked on that text.

    make -C julius_amd/csrc asm                       # leaves gmm_outprob-hip-amdgcn-amd-amdhsa-gfx950.s in csrc/
    tools/gmm_ring_isa.py FILE.s [-o profiles/gmm_ring_loop_isa.txt]

For each instantiation: the per-Gaussian loop (the innermost block holding five s_load_dwordx16) and every other block
with such a load (the prologue) are walked from each load to the next `s_waitcnt lgkmcnt(0)`: that wait has to come
before the block ends, and no instruction in between may name one of the load's sixteen destination registers.  Counts
of the loop (packed operations, waits, s_nop, distance from the youngest load to each wait) are printed with it.

Four instantiations are expected: <NS, HAS_NULL, PULL> for HAS_NULL and PULL false / true.  The per-Gaussian loop of a
PULL instantiation has to show the same packed-operation count, the same waits and the same distances as the plain one
with the same HAS_NULL, and no v_readlane / v_writelane: what the ticket loop needs in SGPRs may be saved outside the
Gaussian loop, never inside it.  The exit status is 1 when the rule or one of these is broken."""
import argparse
import re
import sys

SREG = re.compile(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b")


def sregs(text):
    out = set()
    for m in SREG.finditer(text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def functions(lines):
    name, body = None, []
    for ln in lines:
        m = re.match(r"^(_Z\w*gmm_tile_ring_kernel\w*):", ln)
        if m:
            name, body = m.group(1), []
        elif name and ln.startswith(".Lfunc_end"):
            yield name, body
            name = None
        elif name:
            body.append(ln.rstrip("\n"))


def blocks(body):
    cur, label = [], "entry"
    for ln in body:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            yield label, cur
            cur, label = [], m.group(1)
            continue
        code = ln.split(";")[0].strip()
        if not code or code.startswith("."):
            continue
        cur.append(code)
        if re.match(r"s_c?branch|s_endpgm|s_setpc", code):
            yield label, cur
            cur, label = [], label + "+"
    yield label, cur


def check(label, ins):
    """-> (problems, [packed ops between the youngest load and each wait])"""
    bad, dist, pending, since = [], [], {}, 0
    for i, code in enumerate(ins):
        op = code.split()[0]
        if op == "s_load_dwordx16":
            dst = sregs(code.split(",")[0])
            for k, regs in pending.items():
                if regs & sregs(code):
                    bad.append(f"{label}: `{code}` names a home still in flight (load at {k})")
            pending[i] = dst
            since = 0
        elif code.startswith("s_waitcnt") and "lgkmcnt(0)" in code:
            if pending:
                dist.append(since)
            pending = {}
        else:
            if op.startswith("v_pk_"):
                since += 1
            for k, regs in pending.items():
                if regs & sregs(code):
                    bad.append(f"{label}: `{code}` names a home in flight (load `{ins[k]}`)")
    if pending:
        bad.append(f"{label}: the block ends with {len(pending)} load(s) not waited for")
    return bad, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    report, failed, seen, loops = [], False, 0, {}
    for name, body in functions(open(a.asm).readlines()):
        seen += 1
        report.append(f"==== {name}")
        if any(re.match(r"\s*(v_fma|v_pk_fma|scratch_|buffer_store.*offen)", ln) for ln in body):
            report.append("     FUSED MULTIPLY-ADD OR SCRATCH ACCESS IN THE KERNEL"); failed = True
        for label, ins in blocks(body):
            nload = sum(c.startswith("s_load_dwordx16") for c in ins)
            if not nload:
                continue
            bad, dist = check(label, ins)
            failed |= bool(bad)
            ops = [c.split()[0] for c in ins]
            report.append(f"---- block {label}: {nload} loads, {sum(o.startswith('v_pk_') for o in ops)} packed operations "
                          f"({sum(o in ('v_pk_add_f32', 'v_pk_mul_f32') for o in ops)} v_pk_add/mul_f32), "
                          f"{sum(c.startswith('s_waitcnt') and 'lgkmcnt' in c for c in ins)} lgkmcnt waits, "
                          f"{ops.count('s_nop')} s_nop, {ops.count('s_mov_b32') + ops.count('s_mov_b64')} s_mov, {len(ins)} instructions")
            report.append(f"     packed operations between the youngest load and each wait: {dist}")
            report.append("     rule: " + ("kept" if not bad else "BROKEN"))
            report += ["     " + b for b in bad]
            if nload == 5:
                report += ["\t" + c for c in ins]
                if any(o.startswith(("v_readlane", "v_writelane")) for o in ops):
                    report.append("     SGPR SAVE OR RESTORE INSIDE THE PER-GAUSSIAN LOOP"); failed = True
                m = re.search(r"ILi\d+ELb([01])ELb([01])E", name)     # <NS, HAS_NULL, PULL>
                if m:
                    loops[(m.group(1), m.group(2))] = (sum(o.startswith("v_pk_") for o in ops),
                                                       sum(c.startswith("s_waitcnt") and "lgkmcnt" in c for c in ins), dist)
    if seen != 4:
        report.append(f"expected four instantiations of gmm_tile_ring_kernel, found {seen}"); failed = True
    for null in "01":
        plain, pull = loops.get((null, "0")), loops.get((null, "1"))
        same = plain is not None and plain == pull
        report.append(f"==== HAS_NULL={null}: per-Gaussian loop of the PULL instantiation (packed operations, waits, distances) "
                      f"{pull} vs plain {plain}: " + ("same" if same else "DIFFERENT"))
        failed |= not same
    text = "\n".join(report) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text if not a.out else "\n".join(l for l in report if not l.startswith("\t")) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
