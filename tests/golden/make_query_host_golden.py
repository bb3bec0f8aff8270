"""Writes tests/golden/query_host_parent.json: what the cases of tests/test_gpu_query_host.py launch, grow, return and
write on a build of the commit the query host path was refactored from.  Run once, on a GPU, from a checkout of that
commit with this file and the test module added and the library built:

    python tests/golden/make_query_host_golden.py <commit hash>

The test compares against the file and never writes it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    commit = sys.argv[1]
    assert len(commit) == 40 and all(ch in "0123456789abcdef" for ch in commit), "the full hash of the recorded commit"
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "query_host_parent.json")
    import torch

    import ans_large_alphabet_amd as A
    import test_gpu_query_host as T

    torch.zeros(1, device="cuda")
    cases = T.run_cases(A, torch)
    with open(out, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (out, len(cases)))


if __name__ == "__main__":
    main()
