"""K0c gained a fourth template parameter (KEEP), so profiles/kernel_resources.py --compare, which pairs kernels by their mangled
names, reports every instantiation of mpmpc_car_corridor_kernel as "only in" one build.  This pairs them by what they are:
<W, L, T> of the other build with <W, L, T, false> of this one, and compares table rows and disassembly as --compare does.

    python profiles/commitment/compare_k0c.py OTHER.so      # exit status 1 if a pair differs

It also prints the rows of the KEEP instantiations, which have no partner."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_resources as K

NAME = "mpmpc_car_corridor_kernel<"


def main(other):
    mine = {r["name"]: r for r in K.kernel_table() if r["name"].startswith(NAME)}
    theirs = {r["name"]: r for r in K.kernel_table(other) if r["name"].startswith(NAME)}
    da, db = K.disassembly(), K.disassembly(other)
    bad = 0
    for name, t in sorted(theirs.items()):
        m = mine.get(name[:-1] + ", false>")
        if m is None:
            print("no partner here: %s" % name)
            bad += 1
            continue
        rows = [f for f in ("vgpr", "agpr", "sgpr", "scratch", "lds", "code_bytes") if m[f] != t[f]]
        same = da[m["mangled"]] == db[t["mangled"]]
        print("%-58s -> %-14s table %s, instructions %s" % (name, "<..., false>", "equal" if not rows else "differs in " + ", ".join(rows),
                                                       "identical" if same else "DIFFER"))
        bad += bool(rows) or not same
    print(K.render([r for n, r in sorted(mine.items()) if n.endswith(", true>")]), end="")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
