#!/usr/bin/env python3
"""Compare two gfx950 assembly listings (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/isa_compare.py before.s after.s

For a refactor that must leave the generated code alone.  No GPU, no compiler: the two listings are
parsed as text and instructions are classified by mnemonic prefix only.  For every kernel symbol
(.amdhsa_kernel) the script requires
  * the same set of symbols in both files,
  * identical .amdhsa_next_free_vgpr, .amdhsa_private_segment_fixed_size (scratch) and
    .amdhsa_group_segment_fixed_size,
  * the identical sequence of mnemonics after dropping everything except v_*, ds_*, global_*,
    s_load*, s_waitcnt and s_barrier (every vector, LDS and memory instruction, wait and barrier),
  * the identical FULL mnemonic sequence, scalar instructions included, of every loop body (from a
    label that is the target of a backward branch to that branch).
Scalar ALU / branch instructions outside loops and next_free_sgpr may differ; kernels where they
do are listed with the counts.  Exit status 0 when every requirement holds, 1 otherwise."""
import re
import sys

KEEP = ("v_", "ds_", "global_", "s_load", "s_waitcnt", "s_barrier")
MUST_MATCH = ("next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"^([.\w$]+):")


def parse(path):
    """-> {kernel symbol: {"items": [("label", name) | ("ins", mnemonic, operands)], "meta": {}}}"""
    funcs, meta, cur, kern = {}, {}, None, None
    pending = set()
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            if line.startswith(".type") and line.endswith("@function"):
                pending.add(line.split()[1].split(",")[0])
            elif line.startswith(".amdhsa_kernel"):
                kern, cur = line.split()[1], None
                meta[kern] = {}
            elif line.startswith(".end_amdhsa_kernel"):
                kern = None
            elif kern is not None and line.startswith(".amdhsa_"):
                key, val = line.split(None, 1)
                meta[kern][key[len(".amdhsa_"):]] = val
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif LABEL.match(line):
                name = LABEL.match(line).group(1)
                if name in pending:
                    pending.discard(name)
                    cur = funcs.setdefault(name, [])
                elif cur is not None:
                    cur.append(("label", name))
            elif cur is not None and not line.startswith("."):
                parts = line.split(None, 1)
                cur.append(("ins", parts[0], parts[1] if len(parts) > 1 else ""))
    return {k: {"items": funcs.get(k, []), "meta": m} for k, m in meta.items()}


def loops(items):
    """full mnemonic sequences of the loop bodies, in the order of their closing branches"""
    at = {it[1]: i for i, it in enumerate(items) if it[0] == "label"}
    out = []
    for i, it in enumerate(items):
        if it[0] == "ins" and (it[1].startswith("s_cbranch") or it[1] == "s_branch"):
            j = at.get(it[2].strip())
            if j is not None and j < i:
                out.append(tuple(x[1] for x in items[j:i + 1] if x[0] == "ins"))
    return out


def compare(a, b):
    problems, notes = [], []
    if set(a) != set(b):
        problems.append("symbol sets differ: only before %s, only after %s"
                        % (sorted(set(a) - set(b)), sorted(set(b) - set(a))))
    for k in sorted(set(a) & set(b)):
        ia, ib = a[k]["items"], b[k]["items"]
        for key in MUST_MATCH:
            if a[k]["meta"].get(key) != b[k]["meta"].get(key):
                problems.append("%s: %s %s -> %s" % (k, key, a[k]["meta"].get(key), b[k]["meta"].get(key)))
        ma = [x[1] for x in ia if x[0] == "ins"]
        mb = [x[1] for x in ib if x[0] == "ins"]
        if not ma or not mb:    # (the function label was not found: nothing below would compare anything)
            problems.append("%s: no instructions parsed (%d before, %d after)" % (k, len(ma), len(mb)))
        fa = [m for m in ma if m.startswith(KEEP)]
        fb = [m for m in mb if m.startswith(KEEP)]
        if fa != fb:
            at = next((i for i, (x, y) in enumerate(zip(fa, fb)) if x != y), min(len(fa), len(fb)))
            problems.append("%s: vector/LDS/memory/wait sequence differs at %d of %d/%d: %s | %s"
                            % (k, at, len(fa), len(fb), fa[at:at + 4], fb[at:at + 4]))
        la, lb = loops(ia), loops(ib)
        if la != lb:
            problems.append("%s: loop bodies differ (%d loops before, %d after; first difference: loop %d)"
                            % (k, len(la), len(lb),
                               next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))))
        if ma != mb or a[k]["meta"].get("next_free_sgpr") != b[k]["meta"].get("next_free_sgpr"):
            moved = sum(1 for x, y in zip(ma, mb) if x != y) + abs(len(ma) - len(mb))
            notes.append("%s: %d -> %d instructions, %d positions differ, sgpr %s -> %s"
                         % (k, len(ma), len(mb), moved, a[k]["meta"].get("next_free_sgpr"),
                            b[k]["meta"].get("next_free_sgpr")))
    return problems, notes


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = parse(argv[1]), parse(argv[2])
    problems, notes = compare(a, b)
    print("%d kernels before, %d after" % (len(a), len(b)))
    print("%d kernels differ in scalar code outside loops only (allowed):" % len(notes))
    for n in notes:
        print("  " + n)
    print("%d violations" % len(problems))
    for p in problems:
        print("  " + p)
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
