"""Dev helper: the K loops of the 128 x 128 MFMA tile as the compiler emitted them.

Usage: isa_kloop.py gemm.s [--check]
  gemm.s: hipcc -O3 ... --offload-arch=gfx950 -S --cuda-device-only csrc/kernels_gemm.hip

For each k_gemm128_mfma3 instantiation: the resource line and the interior tile's K loop in
execution order, condensed to
    [n mfma] / ds_read xN / s_waitcnt ... / s_barrier / global_load_lds xN / branches and labels
Runs of scalar and vector ALU between them are folded into "(n salu)" / "(n valu)".
--check: exit 1 unless, in every interior loop,
  * no s_waitcnt lgkmcnt has fewer than 15 MFMAs between it and the last preceding ds_read, except
    the one directly in front of an s_barrier;
  * no run of global_load_lds is longer than two without an MFMA between;
  * nothing but scalar ALU sits between s_barrier and the next MFMA.
"""
import re
import sys


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return "ds_write"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("global_load_lds") or (op.startswith("global_load") and ins.rstrip().endswith(" lds")):
        return "dma"
    if op.startswith("global_load") or op.startswith("global_store") or op.startswith("global_atomic"):
        return "vmem"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def functions(s):
    for m in re.finditer(r'^(_ZN4smlu15k_gemm128_mfma3\S+):', s, re.M):
        i = m.end()
        j = s.find('.Lfunc_end', i)
        yield m.group(1), s[i:j], s[j:j + 6000]


def body_lines(b):
    out = []
    for ln in b.split("\n"):
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith(".") and not ln.endswith(":"):
            continue
        out.append(ln)
    return out


def interior_loop(lines):
    """The interior K loop as executed: the label .. backward-branch span with at least 64 MFMAs, a
    barrier and LDS-DMA that is densest in MFMAs, walked from its header along the hot path (exit
    branches not taken; a forward branch taken when it skips the register staging of the partial
    slice, i.e. MFMA-free code with LDS writes; the back edge taken only where falling through would
    leave the loop)."""
    pos = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    kind = [None if ln.endswith(":") else classify(ln) for ln in lines]
    best = None
    for i, ln in enumerate(lines):
        if kind[i] != "branch":
            continue
        tgt = ln.split()[-1]
        if tgt not in pos or pos[tgt] >= i:
            continue
        seg = kind[pos[tgt]:i + 1]
        if seg.count("mfma") >= 64 and "barrier" in seg and "dma" in seg:
            dens = seg.count("mfma") / len(seg)   # the edge loops carry a branch per MFMA block
            if best is None or dens > best[2]:
                best = (pos[tgt], i, dens)
    if best is None:
        return None, []
    lo, hi = best[:2]
    for i, ln in enumerate(lines):   # the loop may have more than one back edge: span to the last one
        if kind[i] == "branch" and pos.get(ln.split()[-1]) == lo and i > hi:
            inner = [j for j in range(hi + 1, i) if kind[j] == "mfma"]
            if not inner:
                hi = i
    seq, pc, steps = [], lo, 0
    while steps < 20000:
        steps += 1
        ln = lines[pc]
        if ln.endswith(":"):
            if pc == lo and seq:
                break
            seq.append(("label", ln))
            pc += 1
            continue
        k = kind[pc]
        if k != "branch":
            seq.append((k, ln))
            pc += 1
            if pc > hi:
                break
            continue
        tgt = pos.get(ln.split()[-1])
        cond = ln.split()[0] != "s_branch"
        if not cond:
            seq.append((k, ln))
            if tgt == lo:
                break
            pc = tgt
        elif tgt is None or tgt < lo or tgt > hi:
            seq.append((k, ln + "   (exit, not taken)"))
            pc += 1
        elif tgt == lo:
            if pc + 1 > hi:
                seq.append((k, ln))
                break
            seq.append((k, ln + "   (last slice only)"))
            pc += 1
        elif tgt > pc:
            skipped = [x for x in kind[pc + 1:tgt] if x]
            if "ds_write" in skipped and "mfma" not in skipped:
                seq.append((k, ln + "   (taken: skips the partial slice's staging)"))
                pc = tgt
            else:
                seq.append((k, ln + "   (not taken)"))
                pc += 1
        else:
            seq.append((k, ln + "   (not taken)"))
            pc += 1
    return lines[lo], seq


def condense(seq):
    """seq: list of (kind, text) -> list of (kind, count, text)"""
    out = []
    for kind, text in seq:
        if out and out[-1][0] == kind and kind in ("mfma", "ds_read", "ds_write", "dma", "salu", "valu", "vmem"):
            out[-1][1] += 1
        else:
            out.append([kind, 1, text])
    return out


def show(items):
    for kind, n, text in items:
        if kind == "mfma":
            print(f"      [{n} mfma]")
        elif kind in ("ds_read", "ds_write", "vmem"):
            print(f"      {kind} x{n}")
        elif kind == "dma":
            print(f"      global_load_lds x{n}")
        elif kind in ("salu", "valu"):
            print(f"      ({n} {kind})")
        elif kind == "label":
            print(f"    {text}")
        else:
            print(f"      {text}")


def check(items):
    bad = []
    since_read = None   # MFMAs since the last ds_read
    for idx, (kind, n, text) in enumerate(items):
        if kind == "ds_read":
            since_read = 0
        elif kind == "mfma" and since_read is not None:
            since_read += n
        elif kind == "wait" and "lgkmcnt" in text and since_read is not None:
            nxt = next((k for k, _, _ in items[idx + 1:] if k not in ("salu", "label")), None)
            if since_read < 15 and nxt != "barrier":
                bad.append(f"{text}: {since_read} MFMAs after the last ds_read")
        elif kind == "barrier":
            for k, _, t in items[idx + 1:]:
                if k == "mfma":
                    break
                if k not in ("salu", "label"):
                    bad.append(f"{t.split()[0]} between s_barrier and the next MFMA")
                    break
    run = 0
    for kind, n, text in items:
        if kind == "dma":
            run += n
            if run > 2:
                bad.append(f"{run} global_load_lds without an MFMA between")
                run = -10**6
        elif kind == "mfma":
            run = 0
    return bad


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    do_check = "--check" in sys.argv
    s = open(args[0]).read()
    failed = False
    for name, b, tail in functions(s):
        tmpl = re.search(r'mfma3ILb(\d)ELb(\d)ELb(\d)E', name)
        tag = "TRSM=%s EB=%s GATHER=%s" % tmpl.groups() if tmpl else name
        res = {k: re.search(r'; %s: (\d+)' % k, tail) for k in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")}
        print(f"k_gemm128_mfma3<{tag}>  " + "  ".join(f"{k} {v.group(1)}" for k, v in res.items() if v))
        lines = body_lines(b)
        head, seq = interior_loop(lines)
        if head is None:
            print("  no interior loop found")
            failed = True
            continue
        kinds = [k for k, _ in seq]
        items = condense(seq)
        print(f"  interior loop {head} {kinds.count('mfma')} mfma, {kinds.count('ds_read')} ds_read, "
              f"{kinds.count('dma')} global_load_lds, {kinds.count('barrier')} s_barrier")
        show(items)
        if do_check:
            bad = check(items)
            for x in bad:
                print(f"    CHECK FAILED: {x}")
            failed |= bool(bad)
            if not bad:
                print("    check ok")
    sys.exit(1 if failed else 0)


main()
