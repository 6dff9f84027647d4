#!/usr/bin/env python3
"""Extract the vector of the reference's polynomial evaluation test into tests/golden/poly_eval_fixtures.json.

Run once where the reference tree is at hand (environment variable FNFT_REFERENCE, as for
extract_reference_fixtures.py); the output is committed and is all the tests read.  Only NUMBERS are extracted -- the
degree, the four coefficients, the two points (one inside and one outside the unit circle) and the factor of
DBL_EPSILON the test allows -- no source text is kept.  The expected values are restated as a rule.

Source (relative to the reference tree): test/fnft__poly/fnft__poly_eval_test.c:28-83 (both tests use the same
numbers and the same bound)."""
import json
import os
import re

from extract_reference_fixtures import array_init, c2l, read, strip_comments

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    src = strip_comments(read("test/fnft__poly/fnft__poly_eval_test.c"))
    blk = src[src.index("poly_evalderiv_test"):]
    deg = int(re.search(r"deg\s*=\s*(\d+)\s*;", blk).group(1))
    p = array_init(blk, "p")
    z = array_init(blk, "z")
    bounds = set(re.findall(r">\s*(\d+)\s*\*\s*DBL_EPSILON", src))
    assert len(p) == deg + 1 and len(z) == 2 and len(bounds) == 1, (p, z, bounds)
    assert abs(z[0]) < 1.0 < abs(z[1])
    out = {
        "_generated_by": "tests/golden/extract_poly_eval_fixtures.py",
        "poly_eval": {
            "deg": deg, "p": [c2l(x) for x in p], "z": [c2l(x) for x in z],
            "exact": "value[i] = sum_j p[j]*z[i]**(deg-j); deriv[i] = sum_{j>=1} (deg-(j-1))*p[j-1]*z[i]**(deg-j)",
            "metric": "sum_i |x[i] - exact[i]| / sum_i |exact[i]|",
            "bound_dbl_epsilon": int(bounds.pop()),
        },
    }
    with open(os.path.join(HERE, "poly_eval_fixtures.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote poly_eval_fixtures.json:", out["poly_eval"])


if __name__ == "__main__":
    main()
