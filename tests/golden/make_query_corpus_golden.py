"""Writes tests/golden/query_corpus_digest.json: per committed seed the digests of query_model.draw_pool(seed) and of
query_model.case(pool, n) for n < 7 * 12, over a canonical serialisation (query_model.digest).

The committed file was recorded on the commit BEFORE the page calls' generators were added to tests/query_model.py, with
the function bodies of digest / corpus_digest as they stand there: committed failures are replayed by seed and case
number, so every case of the seven calls must stay what it was.  Run it again only where a change of those cases is
intended, and say so: python tests/golden/make_query_corpus_golden.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import query_model as Q  # noqa: E402

if __name__ == "__main__":
    out = dict(calls=list(Q.CALLS), cases_per_seed=len(Q.CALLS) * 12, seeds={str(seed): Q.corpus_digest(seed) for seed in Q.SEEDS})
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "query_corpus_digest.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
