"""Implicit-feedback ALS on the GPU (als_gram_table, als_solve_implicit): the table Gram against its derived bound, every
query against the fp64 restatement of implicit_ref.py, the launch contract, and training on a small grid.

The bounds: the table Gram |G - G_exact|_ij <= n u (|Y|^T |Y|)_ij, the classical dot-product bound, valid for any
summation order (u = 2^-24 / 2^-53; G_exact in extended precision); the ladder rowshapes.BOUND per row (1e-4 fp32, 1e-8
fp64) with empty rows exactly zero; the conditioning block max(BOUND, 3 x the fp32 restatement's recorded worst row of
the case). test_implicit_host.py proves on the CPU, with the restatement alone, that a correct fp32 implementation stays
5 x inside the ladder bound and every mutant (an entry dropped, a rating + 1, lambda n for lambda, b without the 1 +,
G left out) 5 x outside it (3 bars on the conditioning block), for exactly the (k, alpha, lambda) used here. Every case
prints its worst row before it asserts.

Measured on an MI355X: table Gram at n = 5,000 at most 3.4 u (fp32) / 12.5 u (fp64) of the n u bound's unit, i.e.
7e-4 / 2.5e-3 of the bound; ladder worst rows fp32 1.6e-6 .. 2.0e-6 (the fp32 restatement: 4.9e-7 .. 1.15e-6), fp64
1.3e-15 .. 2.6e-15; conditioning fp32 2.1e-5 / 2.7e-5 / 4.3e-5 / 1.05e-4 against bars of 1e-4 / 1e-4 / 1e-4 / 1.47e-4,
fp64 at most 4.8e-14; every width 2.6e-6 (fp32) / 3.4e-15 (fp64) at worst; training: the fp32 factors are 5.1e-5 from the
fp64 restatement after the first half and 1.13e-4 after the fourth iteration (bar 2.7e-4), fp64 7.3e-14. The module
takes 3 s.

Reference semantics: include/als.h (als_solve_implicit). The launch plans are restated in test_implicit_host.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import implicit_ref as ir
import rowshapes as rs
from test_gpu_recommend import expected_topn
from test_implicit_host import gram_table_plan, solve_implicit_plan

pytestmark = pytest.mark.gpu

SIDE_MOVIE, SIDE_USER = 0, 1
SLAB = 256
GRAM_NS = (1, 63, 64, 65, 255, 256, 257, 5000)      # 255 / 257: one slab length -+ 1
GRAM_CASES = [("f32", 10), ("f32", 64), ("f32", 128), ("f64", 10), ("f64", 64), ("f64", 65)]
UNIT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
# rows of the default ladder: degree d at row d - 1, the empty rows at 330 and 343, the long rows from 331
ALONE_ROWS = (0, 31, 32, 329, 331 + rs.LONG_DEGS.index(1025), 331 + rs.LONG_DEGS.index(4000), 330, 343)
WIDTH_ALPHA, WIDTH_LAM = 10.0, 0.1


@pytest.fixture(scope="module")
def gpu(cfk):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


_engines = {}


def engine(cfk, precision, k, table):
    """One engine per (precision, k, table name) with that table as the resident movie factors; never modified."""
    name, F = table
    key = (precision, k, name)
    if key not in _engines:
        with rs.knobs({}):
            eng = cfk.ALSEngine(k, precision)
        eng.alloc_factors(SIDE_MOVIE, len(F))
        eng.write_factors(SIDE_MOVIE, F)
        _engines[key] = eng
    return _engines[key]


def ladder_engine(cfk, precision, k):
    return engine(cfk, precision, k, ("ladder", rs.factors(rs.N_OPP, k)))


def queries(lad, rows=None):
    """The ladder's rows (or the given ones, in that order) as a query CSR."""
    blk = lad.blk
    if rows is None:
        return blk["row_ptr"], blk["col"], blk["ratings"]
    rp = blk["row_ptr"]
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([rp[r + 1] - rp[r] for r in rows])
    idx = np.concatenate([blk["col"][rp[r]:rp[r + 1]] for r in rows] + [np.zeros(0, np.int32)])
    rat = np.concatenate([blk["ratings"][rp[r]:rp[r + 1]] for r in rows] + [np.zeros(0, np.int16)])
    return ptr, idx.astype(np.int32), rat.astype(np.int16)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(tag, got, ref64, degs, bound):
    """Every rated row within `bound` of the oracle, every row without a rating exactly zero; prints the worst row."""
    degs = np.asarray(degs)
    rel = rs.row_errors(got, ref64)
    rated = degs > 0
    i = int(np.nanargmax(np.where(rated, rel, -1.0)))
    print(f"\n[implicit] {tag}: worst row {rel[i]:.3e} (row {i} of {degs[i]} entries), bound {bound:.3e}")
    assert not np.asarray(got)[~rated].any(), "a query without entries is not exactly zero"
    bad = np.nonzero(rated & ~(rel <= bound))[0]
    assert len(bad) == 0, [(int(r), int(degs[r]), float(rel[r])) for r in bad[:12]]
    return rel


# ---------------------------------------------------------------------------------------------------------------------
# 1: the table Gram
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,k", GRAM_CASES, ids=[f"{p}-k{k}" for p, k in GRAM_CASES])
def test_gram_table(gpu, precision, k):
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, precision)
    elem = 4 if precision == "f32" else 8
    try:
        for n in GRAM_NS:
            F = rs.factors(n, k)
            plan = eng.gram_table_plan(n)
            assert plan == gram_table_plan(eng.kp, elem, n) and plan["rows_per_slab"] == SLAB
            eng.alloc_factors(SIDE_MOVIE, n)
            eng.write_factors(SIDE_MOVIE, F)
            G = eng.gram_table(SIDE_MOVIE)
            assert G.shape == (k, k) and G.dtype == eng.np_dtype
            Fx = F.astype(np.longdouble)
            exact = Fx.T @ Fx
            err = np.abs(G.astype(np.longdouble) - exact)
            bound = n * UNIT[precision] * (np.abs(Fx).T @ np.abs(Fx))
            ratio = float((err / bound).max())
            print(f"\n[implicit] gram {precision} k={k} n={n}: max |G - G_exact| / (n u |Y|^T|Y|) = {ratio:.3e} "
                  f"(= {ratio * n:.2f} u), slabs {plan['slabs']}")
            assert (err <= bound).all()
            assert np.array_equal(bits(G), bits(G.T.copy()))                        # exactly symmetric
            assert np.array_equal(bits(eng.gram_table(SIDE_MOVIE)), bits(G))        # repeatable
            # the same rows followed by zero rows up to the next slab boundary
            n_pad = -(-n // SLAB) * SLAB
            if n_pad != n:
                eng.alloc_factors(SIDE_MOVIE, n_pad)
                eng.write_factors(SIDE_MOVIE, F)
                assert eng.gram_table_plan(n_pad)["slabs"] == plan["slabs"]
                assert np.array_equal(bits(eng.gram_table(SIDE_MOVIE)), bits(G))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2: the ladder
# ---------------------------------------------------------------------------------------------------------------------
def run_ladder(cfk, precision, case):
    k, alpha, lam = case
    lad, F, ref64 = ir.ladder_case(*case)
    eng = ladder_engine(cfk, precision, k)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.solve_implicit_plan(344) == solve_implicit_plan(eng.kp, 4 if precision == "f32" else 8, 344, cu)
    got = eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha)
    assert got.shape == (len(lad.degs), k) and got.dtype == eng.np_dtype
    check(f"ladder {precision} k={k} alpha={alpha:g} lam={lam:g}", got, ref64, lad.degs, rs.BOUND[precision])
    return got


@pytest.mark.parametrize("case", ir.LADDER_F32, ids=lambda c: "k%d-a%g-l%g" % c)
def test_ladder_fp32(gpu, case):
    run_ladder(gpu, "f32", case)


@pytest.mark.parametrize("case", ir.LADDER_F64, ids=lambda c: "k%d-a%g-l%g" % c)
def test_ladder_fp64(gpu, case):
    run_ladder(gpu, "f64", case)


# ---------------------------------------------------------------------------------------------------------------------
# 3: conditioning
# ---------------------------------------------------------------------------------------------------------------------
# every case in fp64; in fp32 those whose nearest mutant keeps 3 bars (implicit_ref.COND_F32, test_implicit_host.py)
COND = [("f32", c) for c in ir.COND_F32] + [("f64", c) for c in ir.COND_CASES]


@pytest.mark.parametrize("precision,case", COND, ids=["%s-k%d-a%g-l%g" % ((p,) + c) for p, c in COND])
def test_conditioning(gpu, precision, case):
    k, alpha, lam = case
    lad, F, ref64 = ir.cond_case(*case)
    eng = engine(gpu, precision, k, ("offset", F))
    got = eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha)
    bar = ir.cond_bar(case) if precision == "f32" else rs.BOUND["f64"]
    check(f"conditioning {precision} k={k} alpha={alpha:g} lam={lam:g}", got, ref64, lad.degs, bar)


# ---------------------------------------------------------------------------------------------------------------------
# 4: the contract
# ---------------------------------------------------------------------------------------------------------------------
CONTRACT = [("f32", (64, 10.0, 0.1)), ("f32", (128, 4.0, 0.1)), ("f64", (64, 40.0, 0.05))]


@pytest.mark.parametrize("precision,case", CONTRACT, ids=[f"{p}-k{c[0]}" for p, c in CONTRACT])
def test_batch_independence(gpu, precision, case):
    k, alpha, lam = case
    eng = ladder_engine(gpu, precision, k)
    lad, _, _ = ir.ladder_case(*case)
    n = len(lad.degs)
    assert [int(lad.degs[r]) for r in ALONE_ROWS] == [1, 32, 33, 330, 1025, 4000, 0, 0]
    whole = eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha)
    for r in ALONE_ROWS:
        alone = eng.solve_implicit(SIDE_USER, queries(lad, [r]), lam, alpha)
        assert np.array_equal(bits(alone[0]), bits(whole[r])), (r, int(lad.degs[r]))
    rev = eng.solve_implicit(SIDE_USER, queries(lad, list(range(n - 1, -1, -1))), lam, alpha)
    assert np.array_equal(bits(rev[::-1]), bits(whole))
    assert np.array_equal(bits(eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha)), bits(whole))


def test_more_queries_than_workgroups(gpu):
    """5,000 queries of degrees 1..40 cycling over 512 opposite rows at k = 64: the grid-stride loop reuses a
    workgroup's LDS for several queries, and the longest-first order differs from the order given."""
    k, rows, alpha, lam = 64, 5000, 10.0, 0.1
    lad = rs.anyk_ladder(k, rows)
    F = rs.factors(lad.n_opp, k)
    eng = engine(gpu, "f32", k, ("anyk", F))
    assert eng.solve_implicit_plan(rows)["workgroups"] < rows
    got = eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha)
    sample = list(range(0, rows, 11)) + list(range(rows - 40, rows))
    ref64 = ir.solve_rows(queries(lad, sample), F, lam, alpha)
    check("5000 queries", got[sample], ref64, lad.degs[sample], rs.BOUND["f32"])
    first = eng.solve_implicit(SIDE_USER, queries(lad, list(range(344))), lam, alpha)
    assert np.array_equal(bits(first), bits(got[:344]))


@pytest.mark.parametrize("k", [10, 40])
def test_device_rows(gpu, k):
    n_trained, n_spare, alpha, lam = 30, 20, 10.0, 0.1
    lad = rs.ladder_block((1, 2, 3, 9, 16, 31, 32, 0, 33, 64, 65, 130), n_opp=512, seed=5)
    F = rs.factors(lad.n_opp, k)
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, "f32")
    try:
        eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
        eng.write_factors(SIDE_MOVIE, F)
        U = eng.alloc_factors(SIDE_USER, n_trained + n_spare)
        n_rows = n_trained + n_spare
        pattern = (1000.0 + torch.arange(n_rows * eng.kp, dtype=torch.float32, device=U.device)).reshape(n_rows, eng.kp)
        U[:n_rows].copy_(pattern)                  # every row but the sentinel, padded columns included
        torch.cuda.synchronize()
        before = U.cpu().numpy().copy()
        M_before = eng.factors[SIDE_MOVIE].cpu().numpy().copy()
        rng = np.random.default_rng(8)
        nq = len(lad.degs)
        dst = (n_trained + rng.permutation(n_spare)[:nq]).astype(np.int64)
        got = eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha, dst_rows=dst)
        check(f"device rows k={k}", got, ir.solve_rows(lad.side, F, lam, alpha), lad.degs, rs.BOUND["f32"])
        after = U.cpu().numpy()
        assert np.array_equal(bits(after[dst, :k]), bits(got))
        assert not after[dst, k:].any()
        others = np.setdiff1d(np.arange(n_rows + 1), dst)
        assert np.array_equal(bits(after[others]), bits(before[others]))
        assert not after[n_rows].any()                                          # the sentinel row
        assert np.array_equal(eng.factors[SIDE_MOVIE].cpu().numpy(), M_before)  # the table it sums is only read
        # device rows only: other destinations, no host result
        dst2 = rng.permutation(n_trained)[:nq].astype(np.int64)
        assert eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha, dst_rows=dst2, return_host=False) is None
        after2 = U.cpu().numpy()
        assert np.array_equal(bits(after2[dst2, :k]), bits(got)) and not after2[dst2, k:].any()
        others = np.setdiff1d(np.arange(n_rows + 1), dst2)
        assert np.array_equal(bits(after2[others]), bits(after[others]))
        # out_ld > k: the rows land at that stride and nothing between them is written
        from cfk_amd import _lib
        qp, qi, qr = (np.ascontiguousarray(a) for a in queries(lad))
        wide = np.full((nq, k + 3), 7.0, np.float32)
        st = _lib.lib().als_solve_implicit(eng._h, SIDE_USER, nq, qp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           qi.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           qr.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), ctypes.c_float(lam),
                                           ctypes.c_float(alpha), None, wide.ctypes.data_as(ctypes.c_void_p), k + 3)
        assert st == 0 and np.array_equal(bits(wide[:, :k].copy()), bits(got)) and (wide[:, k:] == 7.0).all()
    finally:
        eng.close()


WIDTHS = ([("f32", k) for k in rs.WIDTH_KS["f32"]] + [("f64", k) for k in rs.WIDTH_KS["f64"] + rs.WIDTH_KS_F64_STRIDES])


@pytest.mark.parametrize("precision,k", WIDTHS, ids=[f"{p}-k{k}" for p, k in WIDTHS])
def test_every_width(gpu, precision, k):
    """Every width next to a stride edge, on both sides, on the width ladder (the 4-entry step, the 64-entry batch
    boundary from both sides, an empty query at the end)."""
    lad = rs.width_ladder()
    F = rs.factors(lad.n_opp, k)
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, precision)
    try:
        eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
        eng.write_factors(SIDE_MOVIE, F)
        got = eng.solve_implicit(SIDE_USER, queries(lad), WIDTH_LAM, WIDTH_ALPHA)
        check(f"width {precision} k={k} (stride {eng.kp})", got, ir.solve_rows(lad.side, F, WIDTH_LAM, WIDTH_ALPHA),
              lad.degs, rs.BOUND[precision])
        G = eng.gram_table(SIDE_MOVIE)
        assert np.array_equal(bits(G), bits(G.T.copy())) and G.shape == (k, k)
    finally:
        eng.close()


@pytest.mark.parametrize("precision,k", [("f32", 10), ("f32", 64), ("f32", 128), ("f64", 64)])
def test_zero_ratings_change_nothing(gpu, precision, k):
    """r = 0 entries -- at the start, inside, at the end and across the 64-entry batch boundary -- leave a query's
    bits those of the query without them."""
    lad = rs.width_ladder()
    F = rs.factors(lad.n_opp, k)
    eng = engine(gpu, precision, k, ("width", F))
    rng = np.random.default_rng(12)
    rp, col, rat = lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"]
    idx, rr, ptr = [], [], [0]
    for i, d in enumerate(lad.degs):
        c, r = list(col[rp[i]:rp[i + 1]]), list(rat[rp[i]:rp[i + 1]])
        for pos in sorted({0, d // 2, d, min(d, 63), min(d, 64)}, reverse=True):
            c.insert(pos, int(rng.integers(0, lad.n_opp)))
            r.insert(pos, 0)
        idx += c
        rr += r
        ptr.append(len(idx))
    plain = eng.solve_implicit(SIDE_USER, queries(lad), WIDTH_LAM, WIDTH_ALPHA)
    padded = eng.solve_implicit(SIDE_USER, (np.asarray(ptr, np.int64), np.asarray(idx, np.int32), np.asarray(rr, np.int16)),
                                WIDTH_LAM, WIDTH_ALPHA)
    rated = lad.degs > 0
    assert np.array_equal(bits(padded[rated]), bits(plain[rated]))
    # a query of zero ratings only has b = 0: the solve runs and gives zeros (of either sign)
    assert not padded[~rated].any()


@pytest.mark.parametrize("precision,k", [("f32", 10), ("f32", 64), ("f64", 64)])
def test_repeated_index_counts_twice(gpu, precision, k):
    lad = rs.repeat_ladder()
    F = rs.factors(lad.n_opp, k)
    eng = engine(gpu, precision, k, ("width", F))
    twice = ir.solve_rows(lad.side, F, WIDTH_LAM, WIDTH_ALPHA)
    once = ir.solve_rows(rs.counted_once(lad.side), F, WIDTH_LAM, WIDTH_ALPHA)
    rep = lad.degs >= 2
    apart = rs.row_errors(once, twice)[rep]
    assert apart.min() >= 5 * rs.BOUND["f32"], apart.min()          # the two models are far apart on these inputs
    got = eng.solve_implicit(SIDE_USER, queries(lad), WIDTH_LAM, WIDTH_ALPHA)
    check(f"repeats {precision} k={k}", got, twice, lad.degs, rs.BOUND[precision])
    assert (rs.row_errors(got, once)[rep] > rs.BOUND["f32"]).all()


def test_between_two_chunks_of_an_explicit_half(gpu):
    k, lam, n_spare = 64, 0.05, 20
    lad, F, _ = ir.ladder_case(64, 10.0, 0.1)
    n = len(lad.degs)
    out = []
    for with_call in (False, True):
        with rs.knobs({}):
            eng = gpu.ALSEngine(k, "f32")
        try:
            eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
            eng.alloc_factors(SIDE_USER, n + n_spare)
            eng.write_factors(SIDE_MOVIE, F)
            eng.set_block(SIDE_USER, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
            assert eng.block_stats(SIDE_USER)["n_reduce"] > 0           # split rows: partial slots are in flight
            eng.set_chunks(SIDE_USER, [0, n // 2, n])
            eng.solve_half_chunk(SIDE_USER, lam, 0)
            if with_call:
                rows = list(range(0, n, 18))
                x = eng.solve_implicit(SIDE_USER, queries(lad, rows), 0.1, 10.0, dst_rows=n + np.arange(len(rows)))
                assert x.shape == (len(rows), k) and len(rows) <= n_spare and x.any()
                assert eng.gram_table(SIDE_MOVIE).shape == (k, k)
            eng.solve_half_chunk(SIDE_USER, lam, 1)
            out.append(eng.read_factors(SIDE_USER, 0, n))
            assert eng.integrity_status() == [0, 0, 0, 0]
        finally:
            eng.close()
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.any(out[0][n // 2:] != 0)


def test_errors(gpu):
    from cfk_amd import _lib
    L = _lib.lib()
    k, lam, alpha = 32, 0.2, 10.0
    lad, F, _ = ir.ladder_case(32, 10.0, 0.2)
    n_user_rows = 8
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, "f32")
        bare = gpu.ALSEngine(k, "f32")
        wide = gpu.ALSEngine(130, "f32")
    qp = np.array([0, 2, 3], np.int64)
    qi = np.array([5, 6, 7], np.int32)
    qr = np.array([1, 2, 3], np.int16)
    out = np.full((2, k), 7.0, np.float32)
    dst = np.array([1, 3], np.int64)

    def p(a, ct):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))

    def raw(e, side=SIDE_USER, n=2, ptr=qp, idx=qi, rat=qr, lam=lam, alpha=alpha, dst_rows=None, host=out, ld=k):
        st = L.als_solve_implicit(e._h, side, n, p(ptr, ctypes.c_int64), p(idx, ctypes.c_int32), p(rat, ctypes.c_int16),
                                  ctypes.c_float(lam), ctypes.c_float(alpha), p(dst_rows, ctypes.c_int64),
                                  None if host is None else host.ctypes.data_as(ctypes.c_void_p), ld)
        return st, L.als_last_error().decode()

    try:
        eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
        eng.write_factors(SIDE_MOVIE, F)
        assert raw(eng)[0] == 0 and not (out == 7.0).any()                      # the valid call the cases vary
        out.fill(7.0)
        st, msg = raw(eng, dst_rows=dst)                                        # dst_rows without this side's factors
        assert st == 5 and "side 1" in msg, msg
        assert raw(bare)[0] == 5                                                # no opposite factors at all
        g = np.zeros((k, k), np.float32)
        assert L.als_gram_table(bare._h, SIDE_MOVIE, g.ctypes.data_as(ctypes.c_void_p), k) == 5
        assert L.als_gram_table(eng._h, SIDE_MOVIE, None, k) == 1
        assert L.als_gram_table(eng._h, SIDE_MOVIE, g.ctypes.data_as(ctypes.c_void_p), k - 1) == 1
        assert L.als_gram_table(eng._h, 2, g.ctypes.data_as(ctypes.c_void_p), k) == 1
        eng.alloc_factors(SIDE_USER, n_user_rows)
        INVALID = [
            ("bad side", dict(side=2), None),
            ("negative n_queries", dict(n=-1), None),
            ("NULL q_ptr", dict(ptr=None), None),
            ("NULL q_idx", dict(idx=None), None),
            ("NULL q_ratings", dict(rat=None), None),
            ("decreasing q_ptr", dict(ptr=np.array([0, 2, 1], np.int64)), "query 1"),
            ("index past the table", dict(idx=np.array([5, 6, lad.n_opp], np.int32)), "query 1"),
            ("negative index", dict(idx=np.array([5, -1, 7], np.int32)), "query 0"),
            ("2^31 entries", dict(ptr=np.array([0, 2, 1 << 31], np.int64)), "2^31"),
            ("both outputs NULL", dict(host=None), None),
            ("out_ld < num_features", dict(ld=k - 1), "out_ld"),
            ("dst row past the table", dict(dst_rows=np.array([1, n_user_rows], np.int64)), "query 1"),
            ("negative dst row", dict(dst_rows=np.array([-1, 2], np.int64)), "query 0"),
            ("repeated dst row", dict(dst_rows=np.array([4, 4], np.int64)), "query 1"),
            ("negative rating", dict(rat=np.array([1, 2, -1], np.int16)), "query 1"),
            ("negative rating in query 0", dict(rat=np.array([1, -3, 2], np.int16)), "query 0"),
            ("lambda 0", dict(lam=0.0), "lambda"),
            ("lambda negative", dict(lam=-0.05), "lambda"),
            ("lambda nan", dict(lam=float("nan")), "lambda"),
            ("lambda inf", dict(lam=float("inf")), "lambda"),
            ("alpha 0", dict(alpha=0.0), "alpha"),
            ("alpha negative", dict(alpha=-1.0), "alpha"),
            ("alpha nan", dict(alpha=float("nan")), "alpha"),
            ("alpha inf", dict(alpha=float("inf")), "alpha"),
        ]
        U_before = eng.factors[SIDE_USER].cpu().numpy().copy()
        for name, kw, needle in INVALID:
            st, msg = raw(eng, **kw)
            assert st == 1, (name, st, msg)
            assert needle is None or needle in msg, (name, msg)
            assert (out == 7.0).all(), name                                     # a failed call writes nothing
            assert np.array_equal(eng.factors[SIDE_USER].cpu().numpy(), U_before), name
        run_ladder(gpu, "f32", (32, 10.0, 0.2))
        assert raw(eng)[0] == 0                                                 # and leaves the engine usable
        good = out.copy()
        out.fill(7.0)
        # widths
        wide.alloc_factors(SIDE_MOVIE, 16)
        st, msg = raw(wide, host=np.zeros((2, 130), np.float32), ld=130)
        assert st == 2 and "128" in msg, msg
        info = (ctypes.c_int64 * 4)()
        assert L.als_solve_implicit_plan(wide._h, 2, info) == 2 and L.als_solve_implicit_plan(eng._h, -1, info) == 1
        assert L.als_solve_implicit_plan(eng._h, 2, None) == 1
        assert L.als_gram_table_plan(wide._h, 16, info) == 2 and L.als_gram_table_plan(eng._h, -1, info) == 1
        assert L.als_gram_table(wide._h, SIDE_MOVIE, np.zeros((130, 130), np.float32).ctypes.data_as(ctypes.c_void_p), 130) == 2
        # nothing to do
        assert raw(eng, n=0, dst_rows=dst)[0] == 0 and raw(eng, n=0, ptr=None, idx=None, rat=None)[0] == 0
        assert (out == 7.0).all() and np.array_equal(eng.factors[SIDE_USER].cpu().numpy(), U_before)
        # a rebased q_ptr: the same two queries behind three unused entries (one of them negative: never read)
        st, _ = raw(eng, ptr=qp + 3, idx=np.concatenate([np.array([9, 9, 9], np.int32), qi]),
                    rat=np.concatenate([np.array([5, 5, 5], np.int16), qr]))
        assert st == 0 and np.array_equal(bits(out), bits(good))
        # the Python wrapper raises the same statuses
        with pytest.raises(gpu.ALSError) as e:
            eng.solve_implicit(SIDE_USER, (qp, qi, np.array([1, 2, -1], np.int16)), lam, alpha)
        assert e.value.status == 1 and "query 1" in str(e.value)
    finally:
        for e in (eng, bare, wide):
            e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5: training
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_training(gpu, precision):
    t = ir.TRAIN
    R, (m, u, r) = ir.train_inputs()
    ds = gpu.Dataset.from_ratings(m, u, r)
    k, lam, alpha = t["k"], t["lam"], t["alpha"]
    app = gpu.ALSApp(1, k, lam, 4, precision=precision, seed=t["seed"]).setup(ds)
    U0 = ds.init_user_factors(k, t["seed"])
    want = ir.train(R, U0, lam, alpha, t["halves"])
    prev = ir.loss(U0, np.zeros((t["n_movies"], k)), R, lam, alpha)
    bound_last = 3 * ir.TRAIN_REF32_DRIFT if precision == "f32" else rs.BOUND["f64"]
    for h in range(t["halves"]):
        app.implicit_half(SIDE_MOVIE if h % 2 == 0 else SIDE_USER, alpha)
        cur = app.implicit_loss(alpha)
        U, M = app.factors()
        assert abs(cur - ir.loss(U, M, R, lam, alpha)) <= 1e-9 * cur          # the app's loss is the helper's
        errs = max(rs.row_errors(U, want[h][0]).max(), rs.row_errors(M, want[h][1]).max())
        print(f"\n[implicit] training {precision} half {h}: loss {cur:.6f} ({100 * (1 - cur / prev):.2f} % lower), "
              f"worst row against the fp64 restatement {errs:.3e}")
        assert cur < prev
        prev = cur
        if precision == "f64":
            assert errs <= rs.BOUND["f64"]
        elif h == 0:
            assert errs <= rs.BOUND["f32"]
        elif h == t["halves"] - 1:
            assert errs <= bound_last
    # recommend on the trained factors: the host top-N of predict's cells
    eng = app.engine
    movie_rows = ds.slots(SIDE_MOVIE, 1)
    rows = ds.slots(SIDE_USER, 1)[:7]
    idx, score = eng.recommend(rows, movie_rows, 5)
    want_idx, want_score = expected_topn(eng.predict(rows, movie_rows), 5)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(score), bits(want_score))
    # one more iteration through implicit_iteration keeps lowering the loss
    app.implicit_iteration(alpha)
    assert app.implicit_loss(alpha) < prev


def test_fold_in_implicit_and_recommend_for(gpu):
    """ALSApp.fold_in_implicit is solve_implicit on foldin_queries' rows, and recommend_for(implicit_alpha=...) recommends
    from those rows; implicit_alpha=None is today's explicit path."""
    t = ir.TRAIN
    R, (m, u, r) = ir.train_inputs()
    ds = gpu.Dataset.from_ratings(m, u, r)
    app = gpu.ALSApp(1, t["k"], t["lam"], 1, precision="f32", seed=t["seed"]).setup(ds, spare_user_rows=2)
    app.implicit_iteration(t["alpha"])
    users = [[(1, 5), (7, 3), (20, 1)], [(3, 2), (48, 4)]]
    movie_rows = ds.slots(SIDE_MOVIE, 1)
    q_ptr, q_idx, q_rat, excl_ptr, excl_idx, _ = gpu.foldin_queries(ds, 1, movie_rows, users)
    M = app.engine.read_factors(SIDE_MOVIE).astype(np.float64)
    X = app.fold_in_implicit(users, t["alpha"])
    check("fold_in_implicit", X, ir.solve_rows((q_ptr, q_idx, q_rat), M, t["lam"], t["alpha"]), np.diff(q_ptr),
          rs.BOUND["f32"])
    base = app.info[SIDE_USER]["n_slots"]
    rows = base + np.arange(2, dtype=np.int64)
    mids, sc = app.recommend_for(users, 5, implicit_alpha=t["alpha"])
    assert np.array_equal(bits(app.engine.read_factors(SIDE_USER, base, 2)), bits(X))
    want_idx, want_score = expected_topn(app.engine.predict(rows, movie_rows), 5, (excl_ptr, excl_idx))
    assert np.array_equal(mids, ds.ids(SIDE_MOVIE)[want_idx]) and np.array_equal(bits(sc), bits(want_score))
    mids_e, _ = app.recommend_for(users, 5)
    assert np.array_equal(bits(app.engine.read_factors(SIDE_USER, base, 2)), bits(app.fold_in(users)))
