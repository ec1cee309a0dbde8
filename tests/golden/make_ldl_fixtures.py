#!/usr/bin/env python3
"""Extract the reference's golden vectors for the LDL^T path into tests/golden/ldl_fixtures.json.

Run in the build container only (it reads /root/reference, which does not exist on the GPU box):
    python tests/golden/make_ldl_fixtures.py

Sources (numbers only — no reference code is copied), all in sprs-ldl/src/lib.rs:
  634-652  test_mat1 (CSC 10 x 10), test_vec1
  654-685  expected_factors1: l_colptr, l_indices, l_data, d
  687-730  expected_lsolve_res1, expected_dsolve_res1, expected_res1
  814-845  permuted_ldl_solve: the 4 x 4 system, its permutation, rhs and solution (cuthill_ldl_solve, 848-866, uses the same system)
Floats are stored as the decimal text of the source, which Python reads to the same double as rustc does."""
import json
import os
import re

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ldl_fixtures.json")


def nums(s):
    return [float(t) if re.search(r"[.eE]", t) else int(t) for t in re.findall(r"-?\d+\.?\d*(?:[eE]-?\d+)?", s)]


def fn_body(src, name):
    m = re.search(r"fn %s\(\)[^{]*\{" % re.escape(name), src)
    assert m, name
    i = m.end()
    depth = 1
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    return src[m.end():i - 1]


def vecs(body):
    """the number lists of every vec![...] of a function body, in order"""
    return [nums(v) for v in re.findall(r"vec!\[(.*?)\]", body, flags=re.S)]


def main():
    src = open(os.path.join(REF, "sprs-ldl", "src", "lib.rs")).read()
    out = {}
    indptr, indices, data = vecs(fn_body(src, "test_mat1"))
    out["mat1"] = {"storage": "csc", "shape": [10, 10], "indptr": indptr, "indices": indices, "data": [float(v) for v in data]}
    out["vec1"] = [float(v) for v in vecs(fn_body(src, "test_vec1"))[0]]
    lp, li, lx, d = vecs(fn_body(src, "expected_factors1"))
    out["factors1"] = {"colptr": lp, "indices": li, "data": [float(v) for v in lx], "d": [float(v) for v in d]}
    for key, fn in (("lsolve1", "expected_lsolve_res1"), ("dsolve1", "expected_dsolve_res1"), ("res1", "expected_res1")):
        out[key] = [float(v) for v in vecs(fn_body(src, fn))[0]]
    body = fn_body(src, "permuted_ldl_solve")
    body = re.sub(r"//[^\n]*", "", body)
    indptr, indices, data, perm, b, x0 = vecs(body)
    out["permuted"] = {"storage": "csc", "shape": [4, 4], "indptr": indptr, "indices": indices, "data": [float(v) for v in data],
                       "perm": perm, "b": [float(v) for v in b], "x": [float(v) for v in x0]}
    assert len(out["mat1"]["indices"]) == 28 and len(out["factors1"]["data"]) == 13 and out["permuted"]["perm"] == [0, 2, 1, 3]
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
