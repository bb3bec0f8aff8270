"""Manual timing of ansx_intersect_ids_dev and ansx_intersect_dev on one warm context: ANSfold-1 on
geom0.02 gaps, default options.  A long list of 64 Mi ids is intersected with drivers of 2^10 .. 2^26 ids, about half of
them members, and one three-list query is run.  A host clock around whole calls (each ends in its own read-back; the
torch route ends in a synchronise), the median of --reps calls; every output is compared with numpy (membership by
np.searchsorted over np.cumsum of the gaps and an equality test, the same sets as np.isin at these sizes).

  --mode after   (default) per driver: intersect_dev over [long, driver]; intersect_ids_dev on the driver's ids as
                 candidates in both forced forms (ANSX_INTERSECT_FORM) and by the default rule; next_geq_dev on the same
                 targets.  Then the sweep that places ANSX_ISECT_FULL_PER_BLOCK: both forced forms of intersect_ids_dev
                 (ids only) over ncand / nblocks = 1/4 .. 1024 in powers of two, random candidates, half of them members;
                 "crossing" is the power of two nearest to where the medians cross.  With --profile (a separate pass) the
                 library's event times of the kernels of one call per form.
  --mode before  what a caller had without these calls: decode_sums_dev of every list, then torch.isin and a masked
                 select, ended by a synchronise.  (Membership is an equality test: the int32 view needs no sign pass;
                 torch.searchsorted would.)  Run it from a checkout of the parent commit with --root, never from the code
                 under test; it uses no call the parent lacks.
Both modes draw the same lists from the same seeds.  --merge FILE adds the cases of an earlier record (the other mode's)
under "merged".

    python tests/tools/bench_intersect.py [--mode after|before] [--root DIR] [--reps 25] [--out FILE] [--merge FILE]
                                          [--profile] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("after", "before"), default="after")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_intersect.json"))
    ap.add_argument("--merge", default="")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--small", action="store_true", help="1/64 of every list (a rehearsal, not a measurement)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    shrink = 64 if args.small else 1
    n = (64 << 20) // shrink
    bi = A.DEFAULT_BLOCK_INTS

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    def kernels(fn):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(5):
            fn()
        got = {kn: round(ms / 5, 4) for kn, ms, _ in ctx.profile_get()}
        ctx.profile(False)
        got["sum_ms"] = round(sum(got.values()), 4)
        return got

    class List:
        """ids (host, uint32, non-decreasing) -> container of their gaps and bases on the device"""

        def __init__(self, ids):
            self.ids, self.n = ids, ids.size
            self.nblocks = (ids.size + bi - 1) // bi
            d = torch.from_numpy(ids.view(np.int32)).cuda()
            self.cont = torch.empty(codec.bound(ids.size) + 64, dtype=torch.uint8, device="cuda:0")
            self.bases = torch.empty(self.nblocks + 1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            self.nb, self.nbases = codec.encode_gaps_bases_dev(d.data_ptr(), ids.size, self.cont.data_ptr(), self.cont.numel(),
                                                               self.bases.data_ptr(), self.bases.numel())
            assert self.nbases == self.nblocks + 1

    def members(sums, cand):
        pos = np.searchsorted(sums, cand, side="left")
        return (pos < sums.size) & (sums[np.minimum(pos, sums.size - 1)] == cand), pos

    gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=3)
    sums = np.cumsum(gaps.cpu().numpy().view(np.uint32), dtype=np.uint64)
    last = int(sums[-1])
    assert last < (1 << 32) - 1, "the list leaves 32 bits"
    sums = sums.astype(np.uint32)
    del gaps
    long_ = List(sums)
    rng = np.random.default_rng(1)

    def draw(m, sort):
        c = np.concatenate([sums[rng.integers(0, n, m // 2)], rng.integers(0, last, m - m // 2, endpoint=True).astype(np.uint32)])
        if sort:
            c.sort()
        else:
            rng.shuffle(c)
        return c

    res = {"mode": args.mode, "workload": "ANSfold-1, %d geom0.02 gaps, block_ints %d" % (n, bi), "blocks": long_.nblocks,
           "container_bytes": long_.nb, "last_id": last, "reps": args.reps, "drivers": {}}
    whole = {}

    def before_route(lists):
        """decode_sums_dev on every list, torch.isin of the shortest in the others, the members selected"""
        for L in lists:
            if id(L) not in whole:
                whole[id(L)] = torch.empty(L.n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def run():
            for L in lists:
                codec.decode_sums_dev(L.cont.data_ptr(), L.nb, whole[id(L)].data_ptr(), L.n)
            order = sorted(range(len(lists)), key=lambda i: (lists[i].n, i))
            drv = whole[id(lists[order[0]])]
            keep = torch.ones(drv.numel(), dtype=torch.bool, device="cuda:0")
            for i in order[1:]:
                keep &= torch.isin(drv, whole[id(lists[i])])
            out = drv[keep]
            torch.cuda.synchronize()
            return out

        return run

    def expected_lists(lists):
        order = sorted(range(len(lists)), key=lambda i: (lists[i].n, i))
        drv = lists[order[0]].ids
        keep = np.ones(drv.size, bool)
        for i in order[1:]:
            keep &= members(lists[i].ids, drv)[0]
        return drv[keep]

    def lists_case(lists):
        exp = expected_lists(lists)
        r = {"n": [L.n for L in lists], "result": int(exp.size)}
        if args.mode == "before":
            run = before_route(lists)
            r["before"] = timed(run)
            r["before_correct"] = bool(np.array_equal(run().cpu().numpy().view(np.uint32), exp))
            return r
        out = torch.empty(max(exp.size, 1), dtype=torch.int32, device="cuda:0")
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        bp, nbases = [L.bases.data_ptr() for L in lists], [L.nbases for L in lists]
        torch.cuda.synchronize()

        def run():
            return codec.intersect_dev(ptrs, nbs, bp, nbases, out.data_ptr(), exp.size)

        r["intersect_dev"] = timed(run)
        r["intersect_dev_correct"] = bool(run() == exp.size and np.array_equal(out[:exp.size].cpu().numpy().view(np.uint32), exp))
        if args.profile:
            r["kernels_intersect_dev"] = kernels(run)
        return r

    def ids_case(cand, forms, with_next_geq):
        m, pos = members(sums, cand)
        eids, eidx, epos = cand[m], np.nonzero(m)[0].astype(np.uint32), pos[m].astype(np.uint64)
        k, nc = int(eids.size), cand.size
        dc = torch.from_numpy(cand.view(np.int32)).cuda()
        oi = torch.empty(max(k, 1), dtype=torch.int32, device="cuda:0")
        ox = torch.empty(max(k, 1), dtype=torch.int32, device="cuda:0")
        op = torch.empty(max(k, 1), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        r = {"candidates": nc, "members": k, "per_block": nc / long_.nblocks,
             "touched_blocks": int(np.unique(np.minimum(pos[pos < n], n - 1) // bi).size)}
        for form in forms:
            ctx.debug_set("ANSX_INTERSECT_FORM", form)

            def run(all_out=False):
                return codec.intersect_ids_dev(long_.cont.data_ptr(), long_.nb, long_.bases.data_ptr(), long_.nbases, dc.data_ptr(),
                                               nc, oi.data_ptr(), ox.data_ptr() if all_out else None,
                                               op.data_ptr() if all_out else None, k)

            name = form or "default"
            r[name] = timed(run)
            r[name + "_correct"] = bool(run(True) == k and np.array_equal(oi[:k].cpu().numpy().view(np.uint32), eids)
                                        and np.array_equal(ox[:k].cpu().numpy().view(np.uint32), eidx)
                                        and np.array_equal(op[:k].cpu().numpy().view(np.uint64), epos))
            if args.profile and form:
                r["kernels_" + name] = kernels(run)
            ctx.debug_set("ANSX_INTERSECT_FORM", None)
        if with_next_geq:
            gp = torch.empty(nc, dtype=torch.int64, device="cuda:0")
            gi = torch.empty(nc, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            r["next_geq"] = timed(lambda: codec.next_geq_dev(long_.cont.data_ptr(), long_.nb, long_.bases.data_ptr(), long_.nbases,
                                                             dc.data_ptr(), nc, gp.data_ptr(), gi.data_ptr()))
            r["selective_minus_next_geq_ms"] = r["selective"]["median_ms"] - r["next_geq"]["median_ms"]
        return r

    drivers = {}
    for lg in (10, 14, 18, 22, 26):
        m = max((1 << lg) // shrink, 16)
        drivers[lg] = List(draw(m, True))
        r = {"lists": lists_case([long_, drivers[lg]])}
        if args.mode == "after":
            r["ids"] = ids_case(drivers[lg].ids, ("selective", "full", None), True)
        res["drivers"]["2^%d" % lg] = r
        print("driver 2^%d done" % lg, file=sys.stderr, flush=True)
    second = List(np.sort(draw(max((1 << 22) // shrink, 64), True)))
    res["three_lists"] = lists_case([long_, drivers[18], second])

    if args.mode == "after":
        sweep = {}
        for e in range(-2, 11):
            nc = max(int(long_.nblocks * 2.0 ** e), 1)
            sweep["2^%d" % e] = ids_case(draw(nc, False), ("selective", "full"), False)
            print("sweep 2^%d done" % e, file=sys.stderr, flush=True)
        res["sweep"] = sweep
        # the power of two nearest to where the medians cross: log-linear between the last ratio selective wins at and the next
        es = list(range(-2, 11))
        d = [np.log(sweep["2^%d" % e]["selective"]["median_ms"] / sweep["2^%d" % e]["full"]["median_ms"]) for e in es]
        wins = [x < 0 for x in d]
        if all(wins):
            res["crossing"] = "selective never loses up to 1024 candidates per block"
        elif not any(wins):
            res["crossing"] = "selective never wins from 1/4 candidate per block"
        else:
            j = max(i for i in range(len(es) - 1) if wins[i] and not wins[i + 1]) if any(wins[i] and not wins[i + 1] for i in range(len(es) - 1)) else None
            if j is None:
                res["crossing"] = "the curves do not cross once from selective to full"
            else:
                x = es[j] + d[j] / (d[j] - d[j + 1])
                res["crossing"] = {"log2_per_block": float(x), "nearest_power_of_two": int(2 ** round(x)) if round(x) >= 0 else 2.0 ** round(x)}
    if args.merge:
        with open(args.merge) as fh:
            res["merged"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
