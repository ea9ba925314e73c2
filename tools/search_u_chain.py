#!/usr/bin/env python3
"""Search for the cheapest addition-subtraction chain of x -> x^u on the cyclotomic subgroup (bn254_vm.h::vm_exp_u), where an inverse is a
conjugation and therefore free, and print the chain description gen_constants.py writes to csrc/bn254_constants.h.

The chains searched are the ones vm_exp_u can run without another workspace element: a table of odd powers of x in the three table slots
(built with e_dst as the one temporary), then a left-to-right pass over signed digits of u drawn from the table and from x itself:
  acc <- table[d0];  repeat: acc <- acc^(2^run);  acc <- acc * table[|d|] (conjugated for d < 0)
with every run at most RUN_MAX = 7 squarings, the limit of one f12_cyclo_sqr_n launch.

Cost = squarings + ratio * products.  `--ratio` is the time of one k_f12_mul launch over the time of one Granger-Scott squaring inside
k_f12_cyclo_sqr_n, taken from a kernel trace of the commit the search is made for (profiles/exp_u_chain_ab.txt part B: 257.9 us / (466.3 us / 4.769) = 2.64).

  python tools/search_u_chain.py                      # the search behind the committed chain: three entries, each at most 33
  python tools/search_u_chain.py --max-entry 65       # the wider search recorded in DESIGN.md section 5.1 (four minutes)
  python tools/search_u_chain.py --entries 4          # what a fourth table entry would buy (it needs a workspace slot the program does not have)
  python tools/search_u_chain.py --check              # exit status 1 unless the chain gen_constants.py encodes is as cheap as the cheapest found
"""
import argparse
import functools
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "snark-bn254-verifier_amd"))
import gen_constants as G  # noqa: E402

U = G.U
RUN_MAX = 7
SLOTS = 3            # table slots of vm_exp_u (bn254_vm.h: VE_UT0..2); e_dst is the one temporary while the table is built


def main_pass(table, ratio, run_max=RUN_MAX):
    """Cheapest digit pass for the table (odd exponents, 1 included).  -> (cost, [(digit, run after it)...] MSB first) or None.
    Right to left: an odd n is a table entry (the pass starts there) or n = (m << z) + d with d = +-entry, 1 <= z <= run_max."""
    entries = sorted(table)

    @functools.lru_cache(maxsize=None)
    def g(n):
        if n in table:
            return 0.0, ((n, 0),)
        best = None
        for e in entries:
            for d in (e, -e):
                r = n - d
                if r <= 0 or r >= 2 * n:     # the rest gets smaller with every digit
                    continue
                z = (r & -r).bit_length() - 1
                if z > run_max:
                    continue
                sub = g(r >> z)
                if sub is None:
                    continue
                c = sub[0] + z + ratio
                if best is None or c < best[0]:
                    head = sub[1][:-1] + ((sub[1][-1][0], z),)
                    best = (c, head + ((d, 0),))
        return best

    return g(U)


def build_table(targets, ratio, max_value, slots=SLOTS, max_ops=7, limit=float("inf")):
    """Cheapest way to the table entries `targets` (without x) from x: steps ('sqr', v, a, k): v = a * 2^k in one launch of k squarings, and
    ('mul', v, a, b, conj): v = a + b or a - b.  At no time more than `slots` + 1 values besides x are alive (the table slots and e_dst).
    -> (cost, steps) or None where none costs less than `limit`."""
    targets = frozenset(targets)
    best = [limit, None]

    def live_ok(steps):
        # a value is alive from the step that makes it to its last use; a table entry stays
        for i in range(len(steps)):
            alive = set()
            for j in range(i + 1):
                v = steps[j][1]
                if v in targets or any(v in (s[2], s[3] if s[0] == "mul" else None) for s in steps[i + 1:]):
                    alive.add(v)
            if len(alive) > slots + 1:
                return False
        return True

    def rec(known, cost, steps):
        missing = len(targets - known)
        if missing == 0:
            if cost < best[0] and live_ok(steps):
                best[0], best[1] = cost, list(steps)
            return
        if len(steps) + missing > max_ops or cost + missing >= best[0]:
            return
        cand = {}
        ks = sorted(known)
        for a in ks:
            for k in range(1, RUN_MAX + 1):
                v = a << k
                if v > max_value:
                    break
                if v not in known and k < cand.get(v, (99,))[0]:
                    cand[v] = (k, ("sqr", v, a, k))
            for b in ks:
                if b > a:
                    break
                for v, conj in ((a + b, False), (a - b, True)):
                    if 0 < v <= max_value and v not in known and ratio < cand.get(v, (99,))[0]:
                        cand[v] = (ratio, ("mul", v, a, b, conj))
        for v, (c, step) in sorted(cand.items(), key=lambda kv: (kv[0] not in targets, kv[1][0])):
            rec(known | {v}, cost + c, steps + [step])

    rec(frozenset([1]), 0.0, [])
    if best[1] is None:
        return None
    steps = []
    for st in best[1]:     # squarings of a value nothing else reads are one run
        p = steps[-1] if steps else None
        if p and st[0] == "sqr" and p[0] == "sqr" and st[2] == p[1] and p[1] not in targets and p[3] + st[3] <= RUN_MAX and \
                not any(p[1] in (s[2], s[3] if s[0] == "mul" else None) for s in best[1] if s is not st):
            steps[-1] = ("sqr", st[1], p[2], p[3] + st[3])
        else:
            steps.append(st)
    return best[0], steps


def count(steps, digits):
    sq = sum(s[3] for s in steps if s[0] == "sqr") + sum(r for _, r in digits)
    mul = sum(1 for s in steps if s[0] == "mul") + len(digits) - 1
    return sq, mul


def search(ratio, max_entry, entries, slots, verbose=False):
    """-> list of (cost, squarings, products, table, build steps, digits), cheapest first"""
    tables = {}
    odds = range(3, max_entry + 1, 2)
    res = []
    bound = None
    for k in range(1, entries + 1):
        for extra in itertools.combinations(odds, k):
            m = main_pass(frozenset((1,) + extra), ratio)
            if m is None or (bound is not None and m[0] + k * ratio >= bound + 1e-9):   # an odd table entry costs at least one product
                continue
            used = sorted({abs(d) for d, _ in m[1]} - {1})
            if tuple(used) not in tables:    # ties with the cheapest so far are kept (they are printed), anything dearer is not looked for
                b = build_table(used, ratio, 2 * max_entry, slots, limit=float("inf") if bound is None else bound + 1.0 - m[0] + 1e-9)
                if b is None:
                    continue
                tables[tuple(used)] = b
            b = tables[tuple(used)]
            if b is None:
                continue
            sq, mul = count(b[1], m[1])
            res.append((sq + ratio * mul, sq, mul, tuple(used), b[1], m[1]))
            if bound is None or res[-1][0] < bound:
                bound = res[-1][0]
                if verbose:
                    print("  ... %.2f: %d squarings + %d products, table %s" % (bound, sq, mul, used), file=sys.stderr)
    res.sort(key=lambda r: (r[0], r[3]))
    out, seen = [], set()
    for r in res:
        if (r[3], r[5]) not in seen:
            seen.add((r[3], r[5])); out.append(r)
    return out


def show(r, ratio):
    cost, sq, mul, table, steps, digits = r
    print("cost %.2f at ratio %.2f: %d squarings + %d products, table {%s}, longest run %d" %
          (cost, ratio, sq, mul, ", ".join("x^%d" % t for t in table), max([r_ for _, r_ in digits] + [s[3] for s in steps if s[0] == "sqr"])))
    print("  table:  " + "; ".join(("x^%d = (x^%d)^(2^%d)" % (s[1], s[2], s[3])) if s[0] == "sqr" else
                                   ("x^%d = x^%d * %s" % (s[1], s[2], ("conj(x^%d)" if s[4] else "x^%d") % s[3])) for s in steps))
    print("  main:   " + " ".join("%+d%s" % (d, " |%d|" % run if run else "") for d, run in digits))


def committed():
    """The chain gen_constants.py encodes, in the form of a search result."""
    c = G.u_chain()
    steps = []
    val = {0: 1}
    for op, dst, a, b in c["build"]:
        if op == 0:
            val[dst] = val[a] << b; steps.append(("sqr", val[dst], val[a], b))
        else:
            val[dst] = val[a] + val[b]; steps.append(("mul", val[dst], val[a], val[b], False))
    digits = tuple(zip(c["digits"], c["runs"]))
    sq, mul = count(steps, digits)
    return sq, mul, tuple(c["table"]), steps, digits


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ratio", type=float, default=2.64, help="time of a product over the time of a squaring (default: 2.64)")
    ap.add_argument("--max-entry", type=int, default=33, help="largest table exponent tried (default: 33)")
    ap.add_argument("--entries", type=int, default=SLOTS, help="table entries besides x (default: 3; more need new workspace slots)")
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--check", action="store_true", help="no search beyond the default one: exit 1 unless the committed chain is the cheapest found")
    a = ap.parse_args()
    sq, mul, table, steps, digits = committed()
    acc = 0
    for d, run in digits:
        acc = (acc + d) << run
    assert acc == U
    print("# committed (gen_constants.py -> csrc/bn254_constants.h, BN_U_CHAIN_*)")
    show((sq + a.ratio * mul, sq, mul, table, steps, digits), a.ratio)
    print("# width-4 signed windows (the chain before): 63 squarings + 16 products = %.2f" % (63 + 16 * a.ratio))
    print("# search: at most %d table entries besides x, each at most %d, runs of at most %d squarings%s" %
          (a.entries, a.max_entry, RUN_MAX, "" if a.entries <= SLOTS else "  (NEEDS %d MORE WORKSPACE SLOT(S))" % (a.entries - SLOTS)))
    res = search(a.ratio, a.max_entry, a.entries, max(SLOTS, a.entries), verbose=True)
    for r in res[:a.top]:
        show(r, a.ratio)
    best = res[0]
    same = best[0] >= sq + a.ratio * mul - 1e-9
    print("# the committed chain is %s" % ("as cheap as the cheapest found" if same else "NOT the cheapest found"))
    if a.check and not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
