#!/usr/bin/env python3
"""Record tests/golden/cache_policy_parent.npz: the factor tables every case of tests/test_gpu_cache_policy.py must
reproduce bit for bit.

  CFK_ALS_LIB=<the parent commit's libcfk_als.so> python tools/record_cache_policy_golden.py [--out FILE]

Run on the GPU with the library of the commit whose results are the standard (without CFK_ALS_LIB: the product build of
this tree). Per recorded case (tests/cache_policy_cases.py, RECORDED) the file holds the movie table after the movie
half (`<case>.M`), the sha256 of the whole user table after the user half (`<case>.U_sha256`) and every 8th user row
(`<case>.U_rows`), plus `lib_sha256`, the library that computed them. The golden pins sums and their order: a cache
policy, a schedule or a layout change must leave it alone, and a change that alters a sum on purpose -- another
accumulation order, another split, another solve -- re-records it with this tool and says so.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cache_policy_parent.npz"))
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before the library)
    import __graft_entry__
    import cache_policy_cases as cp
    cfk = __graft_entry__.load_package()
    from cfk_amd import _lib
    out = {"lib_sha256": np.array(__graft_entry__.sha256_file(_lib.LIB_PATH))}
    for case in cp.RECORDED:
        M, U, facts = cp.run_case(cfk, case)
        assert facts["integrity"] == [0, 0, 0, 0], (case.name, facts)
        M2, U2, _ = cp.run_case(cfk, case)
        assert np.array_equal(M, M2) and np.array_equal(U, U2), f"{case.name}: the library does not repeat itself"
        assert np.isfinite(M).all() and np.isfinite(U).all(), case.name
        for key, v in cp.golden_entry(M, U).items():
            out[f"{case.name}.{key}"] = v
        print(case.name, "M", M.shape, cp.digest(M)[:12], "U", U.shape, cp.digest(U)[:12], facts["path"][0], flush=True)
    np.savez(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes; library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
