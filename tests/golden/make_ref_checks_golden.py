#!/usr/bin/env python3
"""Generates tests/golden/ref_checks.json: the REAL reference's answers (oracle/_ref) on the fixed inputs of the tests
that compare the restatement with it (test_oracle.py's *_vs_reference / *_matches_reference tests and
test_generators.py's live zipf comparison), so that those tests need no compiled reference.  Streams are recorded as
hashes of their canonical (padding-zeroed) bytes, like the other fixtures here.  Run in the authoring container only:
    python tests/golden/make_ref_checks_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))  # the package (test_generators imports it)
import oracle_lib as ol  # noqa: E402
import test_generators as tg  # noqa: E402
import test_oracle as to  # noqa: E402

sha = ol.sha256_of


def main():
    assert ol.have_ref(), "build oracle/_ref first (make -C oracle)"
    doc = {"note": "answers of the compiled reference (oracle/_ref) on the inputs of the tests named by each key"}
    doc["fold_unfold"] = {str(f): sha(to.ref_fold_unfold(f, to.fold_unfold_inputs(f))) for f in (1, 2, 3, 5, 7)}
    rows = []
    for f, trial, freqs, nf, largest in to.adjust_freqs_cases():
        M, b = to.ref_adjust_freqs(freqs, nf, largest)
        rows.append(sha(np.uint64(M), b))
    doc["adjust_freqs"] = rows
    rows = []
    for trial, nf, nsyms, M in to.prelude_cases():
        a = np.zeros(8 * nsyms + 64, dtype=np.uint8)
        bits = ol.C.c_uint32(0)
        ol.oracle().ans_oracle_write_prelude(nf, nsyms, M, a, ol.C.byref(bits))  # (only the count of valid bits)
        b = to.ref_prelude(nf, nsyms, M, bits.value)
        got, back = to.ref_load_prelude(b, nsyms)
        rows.append({"bytes": int(b.size), "sha256": sha(b), "loaded": int(got), "loaded_sha256": sha(back)})
    doc["prelude"] = rows
    doc["streams"] = {}
    for kind in (ol.FOLD, ol.RFOLD):
        for f in (1, 3, 5):
            doc["streams"]["%d-%d" % (kind, f)] = [to.ref_stream(kind, f, d, ol.oracle_encode(kind, f, d)[1])
                                                   for _, _, d in to.stream_cases(kind, f)]
    doc["msb"] = [to.ref_stream(ol.MSB, 0, d, ol.oracle_encode(ol.MSB, 0, d)[1]) for _, _, d in to.msb_cases()]
    doc["ansint"] = [to.ref_stream(ol.INT, 0, d, ol.oracle_encode(ol.INT, 0, d)[1]) for d in to.ansint_cases()]
    doc["pa"] = {}
    for kind, f in ((ol.MSB, 0), (ol.INT, 0), (ol.FOLD, 1), (ol.FOLD, 3)):
        rows = []
        for _, _, d in to.pa_cases():
            _, pinfo, info, _, _ = ol.oracle_pa_encode(kind, f, d)
            rows.append(to.ref_pa_block(kind, f, d, pinfo, info))
        doc["pa"]["%d-%d" % (kind, f)] = rows
    rows = []
    for n, q, seed in tg.ZIPF_LIVE:
        vals, nd, u = ol.ref_zipf_trace(n, q, seed, 20000)
        assert np.array_equal(tg.mt19937_canonical(seed, u.size), u), "uniform stream is not std::mt19937's"
        rows.append({"n": n, "q": q, "seed": seed, "count": int(vals.size), "uniforms": int(u.size), "u01_sha256": sha(u),
                     "values_sha256": sha(vals.astype(np.uint32)), "draws_sha256": sha(nd.astype(np.uint32))})
    doc["zipf_live"] = rows
    with open(os.path.join(HERE, "ref_checks.json"), "w") as fh:
        json.dump(doc, fh, indent=0)
    print("ref_checks.json written")


if __name__ == "__main__":
    main()
