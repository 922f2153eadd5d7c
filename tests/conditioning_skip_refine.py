"""The refinement step switched off, for tests/test_gpu_conditioning.py, run in a child process against the DEBUG build.

ALS_DEBUG_SKIP_REFINE (the tile solve emits the unrefined solution where it would have refined; the flag is read below
the gate only) exists only in collaborative-filtering-kafka_amd/build_debug/libcfk_als.so (CFK_DEBUG_KNOBS), so the
child selects the debug build with CFK_ALS_LIB before the package loads it. For k = 64 and 128 under the default knobs
and a 64-entry chunk, every (family, lambda) of tests/conditioning.py is solved on two engines over the same block, one
created without the knob and one with it. Prints one JSON line per case: the per-row errors of both against the fp64
oracle, the rows whose outputs differ bitwise, and the output of every row below the gate that does not.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch  # noqa: F401
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    from cfk_amd._lib import LIB_PATH
    assert "build_debug" in LIB_PATH, LIB_PATH
    import conditioning as cd
    import rowshapes as rs
    lad = cd.block()
    n = lad.blk["n_rows"]
    for k in (64, 128):
        engines = {}
        for name, env in (("refined", {}), ("unrefined", {"ALS_DEBUG_SKIP_REFINE": "1"})):
            os.environ.pop("ALS_DEBUG_SKIP_REFINE", None)
            os.environ.update(env)
            with rs.knobs({"ALS_CHUNK": str(cd.CHUNK)}):
                eng = cfk.ALSEngine(k, "f32")
            os.environ.pop("ALS_DEBUG_SKIP_REFINE", None)
            eng.alloc_factors(1, lad.n_opp)
            eng.alloc_factors(0, n)
            eng.set_block(0, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
            engines[name] = eng
        path = engines["refined"].block_path(0)
        kinds = cd.kinds_of(k)
        for family in cd.FAMILIES:
            for lam in cd.lambdas(k, family):
                c = cd.case(k, family, lam)
                out = {}
                for name, eng in engines.items():
                    eng.write_factors(1, c.F)
                    eng.solve_half(0, lam)
                    out[name] = eng.read_factors(0, 0, n)
                    assert eng.integrity_status() == [0, 0, 0, 0]
                differ = np.any(out["refined"] != out["unrefined"], axis=1)
                below = cd.gate_pivots(c, kinds) < cd.GATE - cd.GATE_BAND
                print(json.dumps({"k": k, "family": family, "lam": lam, "path": path,
                                  "refined": rs.row_errors(out["refined"], c.ref64).tolist(),
                                  "unrefined": rs.row_errors(out["unrefined"], c.ref64).tolist(),
                                  "differ": differ.tolist(),
                                  "unchanged_below": {int(i): out["unrefined"][i].tolist()
                                                      for i in np.nonzero(below & ~differ)[0]}}), flush=True)
        for eng in engines.values():
            eng.close()


if __name__ == "__main__":
    main()
