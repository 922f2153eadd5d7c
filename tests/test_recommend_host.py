"""CPU side of als_recommend (no kernel launch): the launch plan under the sanitizers, the seen-movies exclusion
builder against a brute-force dictionary, and the bindings.

tests/plan/recommend_plan_check.cpp sweeps cfk::recommend_plan over (n_users 1..2^20, n_cand 1..2^21, top_n 1..64,
kp in {16, 64, 128, 1024}, cu_count in {1, 256}). It is compiled with als_plan.cpp by the host C++ compiler under
AddressSanitizer + UBSan and run as a program of its own, exactly as tests/test_plan_host.py runs plan_check: nothing
is preloaded and no Python runs in the sanitizer run.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_plan_host import CSRC, FLAGS, _compilers


@pytest.fixture(scope="module")
def plan_sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recplan") / "recommend_plan_check")
    srcs = [os.path.join(ROOT, "tests", "plan", "recommend_plan_check.cpp"), os.path.join(CSRC, "als_plan.cpp")]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + ["-I", CSRC] + srcs + ["-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail("no host compiler built recommend_plan_check with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    return json.loads(run.stdout)


def test_plan_sweep_holds_every_invariant(plan_sweep):
    """Segments tile [0, n_cand) exactly with no overlap, all but the last are whole candidate tiles, S >= 1, LDS <= 160
    KiB, the workspace arithmetic does not overflow int64 (UBSan would also stop the program), S = 1 whenever the user
    tiles alone reach cu_count."""
    assert plan_sweep["cases"] == 12 * 11 * 64 * 4 * 2
    assert plan_sweep["failed"] == {}
    assert plan_sweep["split"] > 1000 and plan_sweep["single"] > 1000     # both launch shapes are in the sweep


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("chunks", [1, 4])
def test_seen_exclusions_against_a_dictionary(cfk, tiny_path, world, chunks):
    ds = cfk.Dataset.load_netflix(tiny_path)
    ds.set_slot_chunks(1, chunks)
    m, u, _ = ds.ratings()
    movie_ids, user_ids = ds.ids(0), ds.ids(1)
    movie_slots, user_slots = ds.slots(0, world), ds.slots(1, world)
    slot_of_movie = dict(zip(movie_ids.tolist(), movie_slots.tolist()))
    rated = {}
    for mm, uu in zip(m.tolist(), u.tolist()):
        rated.setdefault(uu, set()).add(slot_of_movie[mm])
    rng = np.random.default_rng(5)
    # a shuffled candidate subset (so some rated movies fall outside it) with a few slots listed twice
    cand = rng.permutation(movie_slots)[: len(movie_slots) * 2 // 3]
    cand = np.concatenate([cand, cand[:7]])
    seen_rows = []
    for rank in range(world):
        rows, ptr, idx = cfk.seen_exclusions(ds, world, rank, cand)
        mine = user_ids[user_ids % world == rank]                      # local-row order = ascending raw id
        assert len(rows) == len(mine) and len(ptr) == len(mine) + 1 and ptr[0] == 0 and ptr[-1] == len(idx)
        assert rows.dtype == np.int64 and ptr.dtype == np.int64 and idx.dtype == np.int32
        assert np.array_equal(rows, user_slots[np.searchsorted(user_ids, mine)])     # the chunk-major layout too
        dropped = 0
        for i, uid in enumerate(mine.tolist()):
            got = idx[ptr[i]:ptr[i + 1]]
            assert np.all(np.diff(got) > 0)                            # strictly ascending
            want = [c for c in range(len(cand)) if int(cand[c]) in rated[uid]]
            assert got.tolist() == want, (rank, uid)
            dropped += len(rated[uid] - set(cand.tolist()))
        assert dropped > 0                                             # rated movies outside the subset were dropped
        seen_rows.append(rows)
    assert len(np.unique(np.concatenate(seen_rows))) == len(user_ids)


def test_headers_declare_and_python_binds_the_calls(cfk):
    from cfk_amd import _lib
    als_h = open(os.path.join(ROOT, "include", "als.h")).read()
    host_h = open(os.path.join(ROOT, "include", "als_host.h")).read()
    assert re.search(r"^int als_recommend\(als_engine\* e,", als_h, flags=re.M)
    assert re.search(r"^int als_recommend_plan\(const als_engine\* e,", als_h, flags=re.M)
    assert re.search(r"^int als_write_recommendations_csv\(", host_h, flags=re.M)
    assert "#define ALS_ABI_VERSION 3" in als_h                        # purely additive
    sigs = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sigs["als_recommend"]) == 10 and len(sigs["als_recommend_plan"]) == 5
    L = _lib.lib()
    assert L.als_recommend.argtypes == sigs["als_recommend"] and L.als_recommend_plan.argtypes is not None
    assert callable(cfk.ALSEngine.recommend) and callable(cfk.ALSEngine.recommend_plan)
    assert callable(cfk.ALSApp.recommend) and callable(cfk.seen_exclusions)


def test_recommendations_writer(cfk, tmp_path):
    """als_write_recommendations_csv: userId,movieId,score lines, padding omitted, the score as the prediction CSV prints
    a cell (checked against als_write_prediction_matrix_csv's text of the same floats)."""
    import ctypes
    from cfk_amd import _lib
    users = np.array([3, 9], np.int64)
    movies = np.array([[5, 2, -1], [7, -1, -1]], np.int64)
    scores = np.array([[4.5, 1e-5, -np.inf], [3.1415927, -np.inf, -np.inf]], np.float32)
    out = tmp_path / "rec.csv"
    _lib.call("als_write_recommendations_csv", str(out).encode(), _lib.ptr(users, ctypes.c_int64), 2, 3,
              _lib.ptr(movies, ctypes.c_int64), _lib.ptr(scores, ctypes.c_float))
    ref = tmp_path / "cells.csv"
    cfk.write_prediction_matrix_csv(str(ref), scores[:, :2])
    cells = ref.read_text().splitlines()[1:]
    c0, c1 = cells[0].split(), cells[1].split()
    assert out.read_text() == f"3,5,{c0[0]}\n3,2,{c0[1]}\n9,7,{c1[0]}\n"


@pytest.mark.parametrize("world", [2, 3])
def test_cli_exclusions_equal_seen_exclusions_when_sharded(cfk, tiny_path, world):
    """als_app --top-n with G > 1 shards: query rows = every user's slot under G shards (ascending id), candidates =
    every movie's slot under G shards (ascending id), exclusions = the UNSHARDED user in-block with each row sorted --
    its columns are dense ascending-id movie indices, which are the candidate positions. Restated here and compared
    with seen_exclusions of every rank (which maps the sharded block's movie slots through the candidate rows)."""
    ds = cfk.Dataset.load_netflix(tiny_path)
    user_ids = ds.ids(1)
    urows, mrows = ds.slots(1, world), ds.slots(0, world)
    blk = ds.shard_block(1, 1, 0)
    assert np.array_equal(blk["row_ids"], user_ids)
    cli = [np.sort(blk["col"][blk["row_ptr"][i]:blk["row_ptr"][i + 1]]) for i in range(len(user_ids))]
    seen = 0
    for rank in range(world):
        rows, ptr, idx = cfk.seen_exclusions(ds, world, rank, mrows)
        dense = np.nonzero(user_ids % world == rank)[0]
        assert np.array_equal(rows, urows[dense]) and np.array_equal(rows, cfk.shard_user_rows(ds, world, rank))
        for i, d in enumerate(dense):
            assert np.array_equal(idx[ptr[i]:ptr[i + 1]], cli[d]), (rank, i)
        seen += len(dense)
    assert seen == len(user_ids)


# ---------------------------------------------------------------------------------------------------------------------
# AlsNative.recommend: a public Java method over the private native recommend0 (integration/jni/cfk_als_jni_recommend.c)
# ---------------------------------------------------------------------------------------------------------------------
def test_jni_recommend_native_matches_its_java_declaration():
    from test_integration_java import JNI_C, JNI_JAVA, JNI_PREFIX, JNI_TYPES, _c_calls, _split_params, _strip
    java = _strip(open(JNI_JAVA).read())
    m = re.search(r"private\s+static\s+native\s+(\w+)\s+recommend0\s*\(([^)]*)\)\s*;", java)
    assert m, "AlsNative.recommend0 is not declared"
    jtypes = [p.rsplit(" ", 1)[0].strip() for p in _split_params(m.group(2))]
    assert m.group(1) == "void"
    assert jtypes == ["long", "long[]", "long[]", "int", "long[]", "int[]", "int[]", "float[]"]
    pub = re.search(r"public\s+static\s+void\s+recommend\s*\(([^)]*)\)\s*\{", java)
    assert pub and [p.rsplit(" ", 1)[0].strip() for p in _split_params(pub.group(1))] == jtypes
    assert java.count("recommend0(") == 2                      # the declaration and the one call, in recommend
    csrc = _strip(open(os.path.join(os.path.dirname(JNI_C), "cfk_als_jni_recommend.c")).read())
    cfun = re.findall(r"JNIEXPORT\s+(\w+)\s+JNICALL\s+(\w+)\s*\(([^)]*)\)\s*\{", csrc)
    assert len(cfun) == 1 and cfun[0][:2] == ("void", JNI_PREFIX + "recommend0")
    ctypes_ = [re.sub(r"\s*\w+$", "", p).replace(" ", "") for p in _split_params(cfun[0][2])]
    assert ctypes_ == ["JNIEnv*", "jclass"] + [JNI_TYPES[t] for t in jtypes]
    call = csrc.index("als_recommend(")
    assert "PrimitiveArrayCritical" not in csrc[:call]          # no critical region is open across the call
    assert _c_calls(csrc, "als_recommend") == [10]              # the header's argument count (_lib.SIGNATURES)
    assert "cfk_als_jni_recommend.c" in open(JNI_C).read()      # built into the shim


def test_jni_recommend_length_errors_before_the_abi(cfk):
    """Through the mock JVM, no GPU: every wrong array length is an IllegalArgumentException naming the array, thrown
    before any C ABI call (the engine handle is 0)."""
    from test_jni_shim import JNI_LIB, JavaException, MockJVM
    cfk._lib.lib()
    assert os.path.exists(JNI_LIB)
    jvm = MockJVM()
    bind_recommend0(jvm)
    i64, i32, f32 = (lambda n: jvm.array(np.zeros(n, np.int64))), (lambda n: jvm.array(np.zeros(n, np.int32))), \
        (lambda n: jvm.array(np.zeros(n, np.float32)))
    cases = [((i64(3), i64(5), 2, None, None, i32(5), f32(6)), "outIdx.length"),
             ((i64(3), i64(5), 2, None, None, i32(6), f32(7)), "outScore.length"),
             ((i64(3), i64(5), 2, i64(3), i32(1), i32(6), f32(6)), "exclPtr.length"),
             ((i64(3), i64(5), 2, i64(4), None, i32(6), f32(6)), "both be given"),
             ((i64(3), i64(5), 2, None, i32(1), i32(6), f32(6)), "both be given"),
             ((i64(3), i64(5), 2, jvm.array(np.array([0, 1, 2, 9], np.int64)), i32(2), i32(6), f32(6)), "outside exclIdx")]
    for args, what in cases:
        with pytest.raises(JavaException) as ei:
            jvm.call("recommend0", 0, *args)
        assert ei.value.cls == "java/lang/IllegalArgumentException" and what in ei.value.msg, (what, ei.value)
    with pytest.raises(JavaException) as ei:                    # right lengths, NULL engine: the ABI's own status
        jvm.call("recommend0", 0, i64(3), i64(5), 2, None, None, i32(6), f32(6))
    assert ei.value.cls == "org/apache/kafka/streams/errors/StreamsException" and "als_recommend: als_status 1" in ei.value.msg
    st = jvm.stats()
    assert st["violations"] == 0 and st["open_critical"] == 0 and st["critical"] == 0


def bind_recommend0(jvm):
    """ctypes signature of the recommend0 native on a MockJVM's library (after JNIEnv*, jclass)."""
    import ctypes
    from test_jni_shim import PREFIX
    v, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    fn = getattr(jvm.L, PREFIX + "recommend0")
    fn.restype = None
    fn.argtypes = [v, v, i64, v, v, i, v, v, v, v]
