"""Static census of the loops of a solve kernel in the gfx950 code object of a libmpmpc.so: every backward branch closes a loop;
for each loop its nesting depth, instructions and VALU instructions (v_*), and how many loops it contains.

    python profiles/ipm_passes/census.py [LIB.so] [--kernel 'mpmpc_reduced_kernel<32, 16, false>'] [--min 300]
    python profiles/ipm_passes/census.py --table PARENT.so [LIB.so]      # the tables of docs/HISTORY.md, parent against LIB

The interior-point iteration of ReducedSolver::ipm3 is the loop that holds the factorisation and the two KKT solves: the
largest loop nested in the attempt loop.  With the passes as a run-time loop it contains one inner loop (the pass body, run
twice per iteration: VALU per iteration = loop + one more trip of the inner body); with the passes straight-line it contains
none.  A static count: no GPU involved."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_resources as KR  # noqa: E402


def instructions(so, kernel):
    """[(address, mnemonic, branch target or None)] of the kernel `kernel` (demangled name) in `so`"""
    rows = [r for r in KR.kernel_table(so) if r["name"] == kernel]
    if not rows:
        raise SystemExit("no kernel %r in %s" % (kernel, so))
    txt = KR._run(os.path.join(KR.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + rows[0]["mangled"],
                  KR.code_object(so))
    out = []
    for l in txt.splitlines():
        m = re.match(r"\s*([0-9a-f]+):\s+(\S+)(.*)$", l) or re.match(r"\s*(\S+)(.*?)//\s*([0-9A-Fa-f]+):", l)
        if not m:
            continue
        if m.re.pattern.startswith(r"\s*([0-9a-f]+):"):
            addr, mn, rest = int(m.group(1), 16), m.group(2), m.group(3)
        else:
            mn, rest, addr = m.group(1), m.group(2), int(m.group(3), 16)
        t = re.search(r"<[^>+]*\+0x([0-9a-fA-F]+)>", l)
        out.append((addr, mn, None if t is None or not mn.startswith(("s_cbranch", "s_branch")) else int(t.group(1), 16)))
    base = out[0][0]
    return [(a - base, mn, t) for a, mn, t in out]


def loops(ins):
    """[{start, end, n, valu, depth, inner}] - one per loop header (backward branches to the same address are one loop)"""
    idx = {a: i for i, (a, _, _) in enumerate(ins)}
    span = {}
    for i, (a, mn, t) in enumerate(ins):
        if t is not None and t <= a and t in idx:
            span[idx[t]] = max(span.get(idx[t], 0), i)
    ls = [dict(start=s, end=e, n=e - s + 1, valu=sum(ins[k][1].startswith("v_") for k in range(s, e + 1))) for s, e in sorted(span.items())]
    for l in ls:
        l["depth"] = sum(o["start"] <= l["start"] and l["end"] <= o["end"] for o in ls) - 1
        l["inner"] = [o for o in ls if o is not l and l["start"] <= o["start"] and o["end"] <= l["end"]]
    return ls


def iteration(so, kernel):
    """The interior-point iteration: the largest loop at depth >= 1.  -> dict(valu, total: per iteration, inner body counted
    twice if it is there; inner = number of loops inside)"""
    ins = instructions(so, kernel)
    cand = [l for l in loops(ins) if l["depth"] >= 1]
    it = max(cand, key=lambda l: l["n"])
    # the pass loop is the inner loop that closes last (the other backward branch inside the iteration of the loop form
    # overlaps it without being nested in it: block placement, not a loop of the source)
    direct = sorted(it["inner"], key=lambda o: o["end"])[-1:]
    return dict(valu=it["valu"] + sum(o["valu"] for o in direct), total=it["n"] + sum(o["n"] for o in direct),
                loop_valu=it["valu"], loop_total=it["n"], inner=[(o["n"], o["valu"]) for o in it["inner"]],
                kernel_total=len(ins), kernel_valu=sum(mn.startswith("v_") for _, mn, _ in ins))


ITERATION_KERNELS = ["mpmpc_reduced_kernel<32, 16, false>", "mpmpc_reduced_kernel<16, 16, false>", "mpmpc_reduced_kernel<64, 32, false>",
                     "mpmpc_reduced_t_kernel<64, 32>", "mpmpc_reduced_t_kernel<64, 16>"]


def table(parent, so):
    """markdown: the interior-point iteration of ITERATION_KERNELS and the resources of every kernel whose code changed,
    parent build against `so`"""
    out = ["| kernel | VALU per iteration (parent -> new) | instructions per iteration | loops inside the iteration |", "|---|---|---|---|"]
    for k in ITERATION_KERNELS:
        a, b = iteration(parent, k), iteration(so, k)
        out.append("| `%s` | %d + %d = %d -> %d | %d + %d = %d -> %d | %d -> %d |" % (
            k, a["loop_valu"], a["valu"] - a["loop_valu"], a["valu"], b["valu"], a["loop_total"], a["total"] - a["loop_total"], a["total"], b["total"],
            len(a["inner"]), len(b["inner"])))
    mine, theirs = ({r["name"]: r for r in KR.kernel_table(p)} for p in (so, parent))
    da, db = KR.disassembly(so), KR.disassembly(parent)
    out += ["", "| kernel | registers | scratch (B) | code (B) |", "|---|---|---|---|"]
    for n in sorted(mine):
        m, t = mine[n], theirs[n]
        if da[m["mangled"]] != db[t["mangled"]]:
            out.append("| `%s` | %d -> %d | %d -> %d | %d -> %d |" % (n, t["vgpr"], m["vgpr"], t["scratch"], m["scratch"], t["code_bytes"], m["code_bytes"]))
    out.append("")
    out.append("%d kernels, %d with identical instructions" % (len(mine), sum(da[mine[n]["mangled"]] == db[theirs[n]["mangled"]] for n in mine)))
    return "\n".join(out)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        print(table(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else KR.SO))
        sys.exit(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("so", nargs="?", default=KR.SO)
    ap.add_argument("--kernel", default="mpmpc_reduced_kernel<32, 16, false>")
    ap.add_argument("--min", type=int, default=300, help="list loops of at least this many instructions")
    a = ap.parse_args()
    ins = instructions(a.so, a.kernel)
    print("%s: %d instructions, %d VALU" % (a.kernel, len(ins), sum(mn.startswith("v_") for _, mn, _ in ins)))
    for l in loops(ins):
        if l["n"] >= a.min:
            print("  %sloop @%d..%d: %d instructions, %d VALU, %d loops inside" % ("  " * l["depth"], l["start"], l["end"], l["n"], l["valu"], len(l["inner"])))
    print("interior-point iteration:", iteration(a.so, a.kernel))
