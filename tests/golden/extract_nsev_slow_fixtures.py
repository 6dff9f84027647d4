#!/usr/bin/env python3
"""Extract the reference's second focusing test case (SECH_FOCUSING2, the one its slow-discretization tests use) into
tests/golden/nsev_slow_fixtures.json.

Run once where the reference tree is at hand (environment variable FNFT_REFERENCE, as for
extract_reference_fixtures.py); the output is committed and is all the tests read.  Only NUMBERS are extracted -- the interval, the xi-grid, the 16 values of the reflection
coefficient and the 32 values of a and b -- no source text is kept.  The signal is restated as a rule.

Source (relative to the reference tree): src/private/fnft__nsev_testcases.c:289-461.
The per-file stage lists and error bounds of the slow test files are in reference_fixtures.json["nsev_error_bounds"]
(extract_reference_fixtures.py)."""
import json
import os
import re

from extract_reference_fixtures import c2l, ceval, read, strip_comments

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    src = strip_comments(read("src/private/fnft__nsev_testcases.c"))
    starts = [m.start() for m in re.finditer(r"case nsev_testcases_SECH_FOCUSING2\s*:", src)]
    blk = None
    for i in starts:      # the label also appears in the switch over M; take the block that assigns values
        j = src.index("case nsev_testcases_", i + 10)
        if "contspec_ptr)[0]" in src[i:j]:
            blk = src[i:j]
    assert blk is not None

    def assigns(ptr):
        vals = {}
        for m in re.finditer(r"\(\*" + ptr + r"\)\[(\d+)\]\s*=\s*([^;]+);", blk):
            vals[int(m.group(1))] = ceval(m.group(2))
        return [c2l(vals[i]) for i in range(len(vals))]

    def pair(name):
        a = re.search(name + r"\[0\]\s*=\s*([^;]+);", blk).group(1)
        b = re.search(name + r"\[1\]\s*=\s*([^;]+);", blk).group(1)
        return [ceval(a).real, ceval(b).real]

    out = {
        "_generated_by": "tests/golden/extract_nsev_slow_fixtures.py",
        "nsev_sech_focusing2": {
            "signal": "q[i] = 5.4*sech(t)*exp(-6j*t), t = T0 + i*(T1-T0)/(D-1)",
            "T": pair("T"), "XI": pair("XI"), "M": 16, "kappa": 1,
            "contspec": assigns("contspec_ptr"),
            "ab": assigns("ab_ptr"),
        },
    }
    fx = out["nsev_sech_focusing2"]
    assert len(fx["contspec"]) == 16 and len(fx["ab"]) == 32, (len(fx["contspec"]), len(fx["ab"]))
    with open(os.path.join(HERE, "nsev_slow_fixtures.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote nsev_slow_fixtures.json:", fx["T"], fx["XI"])


if __name__ == "__main__":
    main()
