"""Randomised soak of the nine query calls against the evaluator of tests/query_model.py (manual tool, not collected by pytest):

    SOAK_SECONDS=240 SOAK_SEED=101 python tests/tools/soak_queries.py     # on an MI355X box: seeds 101 and 102, half the time each
    python tests/tools/soak_queries.py --seed 11 --case 37                 # replays one case, under every form of its call
    python tests/tools/soak_queries.py --seed 11 --page-case 5             # replays one case of the two page calls, likewise
    SOAK_PAGE=1 SOAK_SECONDS=240 python tests/tools/soak_queries.py        # the soak over the page cases 0, 1, 2, ...

The generators and the evaluator are those of tests/test_gpu_query_fuzz.py: per seed one pool of 48 lists (query_model.draw_pool)
and the cases 0, 1, 2, ... of that seed (query_model.case: the call is CALLS[n % 7], the first cases of a call carry its planted
errors, later ones draw them).  Case n runs under the default form and under form n // 7 of its call's cycle (FORMS of the test
file); every output array, count, offset and error field is compared with the evaluator and the two runs byte for byte.  The
page cases (query_model.page_case: ansx_topk_facets_batch_dev, ansx_topk_filter_batch_dev) have a numbering of their own and run
through run / judge / PAGE_FORMS of tests/test_gpu_query_fuzz_page.py, totals and facet rows included.  One
process, one time limit, no retry: it stops at the first mismatch, and at the first HIP error, abort or fault, and prints the case.

Run on one MI355X (the calls as of ansx_topk_scored_batch_dev): SOAK_SECONDS=240 SOAK_SEED=101, seeds 101 and 102, 120 s each:
7945 iterations (4071 + 3874), per call intersect 1136, union 1136, bool 1136, topk 1135, topk_bool 1134, topk_query 1134,
topk_scored 1134; plants: 175 overflows of an id of R(q), 81 of a rejected id, 45 terms above ndocs; 0 failures.  (A first run,
whose worked-out group budget mostly gave one group, had 8053 iterations on the same seeds, 0 failures.)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402

torch.zeros(1).cuda()
import ans_large_alphabet_amd as A  # noqa: E402
import query_model as Q  # noqa: E402
import test_gpu_query_fuzz as F  # noqa: E402
import test_gpu_query_fuzz_page as FP  # noqa: E402


def one_case(ctx, G, n, forms):
    """-> the case; raises on the first difference"""
    B = Q.case(G["pool"], n)
    E = F.expected(G, B)
    cap = F.total_of(B, E)
    ref = F.run(torch, ctx, G, B, cap=cap)
    F.judge(G, B, E, ref)
    for keys in forms(B):
        got = F.run(torch, ctx, G, B, keys=keys, cap=cap)
        F.judge(G, B, E, got, keys)
        assert F.image(got) == F.image(ref), F.describe(G, B, keys) + ": not the bytes of the default form"
    return B


def one_page_case(ctx, G, n, forms):
    """-> the page case; raises on the first difference"""
    B = Q.page_case(G["pool"], n)
    ref = FP.run(torch, ctx, G, B)
    FP.judge(G, B, FP.expected(G, B), ref)
    for keys in forms(B):
        E = FP.expected(G, B, keys)  # (which query an error names depends on the keys' budget)
        got = FP.run(torch, ctx, G, B, keys=keys)
        FP.judge(G, B, E, got, keys)
        assert E["status"] != "ok" or FP.image(got) == FP.image(ref), FP.describe(G, B, keys) + ": not the bytes of the default form"
    return B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--page-case", type=int, default=None)
    args = ap.parse_args()
    ctx = A.Context(0)
    if args.page_case is not None:
        seed = args.seed if args.seed is not None else int(os.environ.get("SOAK_SEED", "1"))
        G = FP.page_pool(A, torch, ctx, seed)
        B = one_page_case(ctx, G, args.page_case, lambda B: FP.PAGE_FORMS[B["call"]])
        print("page case", args.page_case, "of seed", seed, "passes:", FP.describe(G, B))
        for i, q in enumerate(B["queries"]):
            print("  query", i, q, "clauses", B["clauses"][i])
        return 0
    if args.case is not None:
        seed = args.seed if args.seed is not None else int(os.environ.get("SOAK_SEED", "1"))
        G = F.device_pool(A, torch, ctx, seed)
        B = one_case(ctx, G, args.case, lambda B: F.FORMS[B["call"]])
        print("case", args.case, "of seed", seed, "passes:", F.describe(G, B))
        for i, q in enumerate(B["queries"]):
            print("  query", i, q)
        return 0
    first = args.seed if args.seed is not None else int(os.environ.get("SOAK_SEED", "1"))
    budget = float(os.environ.get("SOAK_SECONDS", "240"))
    page = os.environ.get("SOAK_PAGE", "") not in ("", "0")
    total, per_call, plants = 0, {c: 0 for c in (Q.PAGE_CALLS if page else Q.CALLS)}, {}
    for seed in (first, first + 1):
        t0 = time.time()
        G = FP.page_pool(A, torch, ctx, seed) if page else F.device_pool(A, torch, ctx, seed)
        n = 0
        while time.time() - t0 < budget / 2:
            try:
                if page:
                    B = one_page_case(ctx, G, n, lambda B: [FP.PAGE_FORMS[B["call"]][(n // len(Q.PAGE_CALLS)) % len(FP.PAGE_FORMS[B["call"]])]])
                else:
                    B = one_case(ctx, G, n, lambda B: [F.FORMS[B["call"]][(n // len(Q.CALLS)) % len(F.FORMS[B["call"]])]])
            except BaseException as e:  # a mismatch, a HIP error, anything: the first one ends the run
                print("FAIL seed", seed, "case", n, "->", type(e).__name__, e)
                print("SOAK stopped: iterations", total, "per call", per_call)
                sys.stdout.flush()
                return 1
            total += 1
            per_call[B["call"]] += 1
            key = B["plant"] and B["plant"][0]
            plants[key] = plants.get(key, 0) + 1
            n += 1
            if n % 100 == 0:
                print("seed", seed, "case", n, "elapsed %.0f s" % (time.time() - t0))
                sys.stdout.flush()
        print("seed", seed, "cases", n, "in %.0f s" % (time.time() - t0))
    print("SOAK done: iterations", total, "fails 0 per call", per_call, "plants", plants)
    return 0


if __name__ == "__main__":
    sys.exit(main())
