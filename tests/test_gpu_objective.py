"""als_implicit_objective on the GPU: every part of every query against the float64 restatement of objective_ref.py
(evaluated on the table's actual values and on the device's own G) within the derived bounds, independence of the batch,
the launch contract, and the loss of a training run against the host's dense-grid loss.

The bounds, with u = 2^-53 (objective_ref.py derives them; none is measured):
    quad     (2k + 2) u |x|^T |G| |x|
    ridge    (k + 2) u lambda x^T x
    observed (2k + n + 8) u sum_e [(1 + alpha r_e)(p_e + a_e)^2 + a_e^2],  a_e = sum_f |x_f| |y_ef|
    totals[3]  (k + 2) u lambda tr|G|
test_objective_host.py proves on the CPU that every mutant of the restatement (an entry dropped, a rating + 1, -s^2 left
out, p = 1 for r = 0, alpha r for 1 + alpha r, G left out or its diagonal only, lambda n for lambda) moves every row it
changes by at least 100 of these bounds on exactly the inputs used here. Every case prints its worst row before it
asserts.

Measured on an MI355X (one box, one run), as the worst fraction of each bound over all cases of a test
(quad / observed / ridge / lambda tr G):
    ladder, solved and random rows   0.143 / 0.026 / 0.215 / 0.105
    5,000 queries                    0.0064 / 0.016 / 0.036 / 0
    stride edges, 21 widths          0.053 / 0.023 / 0.116 / 0.071
    zero ratings and repeated items  0.100 / 0.026 / 0.152 / 0.019
    training, device loss against the host's dense loss: fp64 at most 9.1e-13 absolute = 4.1e-4 of the tolerance, fp32 at
    most 1.2e-4 absolute = 3.7e-3 of the tolerance; smallest rise of f at x +- d over f at the stored row 7.1e-2
The module takes 4 s.

Reference semantics: include/als.h (als_implicit_objective). The launch plan is restated in test_objective_host.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import implicit_ref as ir
import objective_ref as ob
import rowshapes as rs
from test_gpu_implicit import ALONE_ROWS, SIDE_MOVIE, SIDE_USER, bits, queries
from test_objective_host import objective_plan

pytestmark = pytest.mark.gpu

LADDER = ([("f32", c) for c in ob.LADDER_F32 if c != (128, 1.0, 0.1)] +
          [("f64", c) for c in ob.LADDER_F64[:2] + ((65, 40.0, 0.05),) + ob.LADDER_F64[2:]])
LADDER_IDS = ["%s-k%d-a%g-l%g" % ((p,) + c) for p, c in LADDER]
EDGE_KS = (15, 16, 17, 31, 33, 63, 127, 128)
EDGES = [("f32", k) for k in EDGE_KS] + [("f64", k) for k in EDGE_KS + (65, 80, 81, 112, 113)]
EDGE_ALPHA, EDGE_LAM = 10.0, 0.1
NAMES = ("quad", "observed", "ridge")


@pytest.fixture(scope="module")
def gpu(cfk):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


def make_engine(cfk, precision, k, F, n_user_rows):
    with rs.knobs({}):
        eng = cfk.ALSEngine(k, precision)
    eng.alloc_factors(SIDE_MOVIE, len(F))
    eng.write_factors(SIDE_MOVIE, F)
    eng.alloc_factors(SIDE_USER, n_user_rows)
    return eng


def check(tag, eng, qs, rows, lam, alpha, got=None):
    """Every part of every query within its bound of the restatement on the table's actual values and the device's G;
    the totals the ordered host sums of the parts bit for bit; totals[3] within its bound. Prints the worst fractions."""
    k = eng.k
    rows = np.asarray(rows, np.int64)
    if got is None:
        got = eng.implicit_objective(SIDE_USER, qs, rows, lam, alpha, parts=True)
    X = eng.read_factors(SIDE_USER).astype(np.float64)[rows]
    Y = eng.read_factors(SIDE_MOVIE).astype(np.float64)
    G = eng.gram_table(SIDE_MOVIE).astype(np.float64)
    want, bound = ob.parts(qs, X, Y, G, lam, alpha)
    parts = got["parts"]
    assert parts.shape == want.shape and parts.dtype == np.float64
    err = np.abs(parts - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = [int(np.argmax(frac[:, c])) for c in range(3)]
    lam_tr = float(np.float32(lam)) * float(np.trace(G.astype(np.longdouble)))
    tr_bound = (k + 2) * ob.U * float(np.float32(lam)) * float(np.trace(np.abs(G)))
    tr_frac = abs(got["ridge_opp"] - lam_tr) / tr_bound
    print(f"\n[objective] {tag}: worst fraction of the bound " +
          ", ".join(f"{NAMES[c]} {frac[worst[c], c]:.3e} (query {worst[c]})" for c in range(3)) +
          f", lambda tr G {tr_frac:.3e}")
    assert (frac <= 1).all(), [(int(q), int(c), float(parts[q, c]), float(want[q, c]), float(bound[q, c]))
                               for q, c in zip(*np.nonzero(~(frac <= 1)))][:12]
    empty = np.diff(np.asarray(qs[0])) == 0
    assert not parts[empty, 1].any()                      # a query without entries: a middle part of exactly 0
    sums = [0.0, 0.0, 0.0]
    for q in range(len(parts)):                            # ascending query order, in double
        for c in range(3):
            sums[c] += float(parts[q, c])
    assert [got["quad"], got["observed"], got["ridge"]] == sums
    assert got["loss"] == got["quad"] + got["observed"] + got["ridge"] + got["ridge_opp"]
    assert tr_frac <= 1
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1: the ladder -- solved rows, random rows, the minimiser, independence of the batch
# ---------------------------------------------------------------------------------------------------------------------
_ladders = {}


def ladder_state(cfk, precision, case):
    """One engine per ladder case: user rows [0, n) the rows solve_implicit stored, [n, 2n) random rows, [2n, 3n) and
    [3n, 4n) the solved rows +- a seeded perturbation of relative size 1e-2. Read-only afterwards."""
    key = (precision, case)
    if key not in _ladders:
        k, alpha, lam = case
        lad, F, _ = ir.ladder_case(*case)
        n = len(lad.degs)
        eng = make_engine(cfk, precision, k, F, 4 * n)
        eng.solve_implicit(SIDE_USER, queries(lad), lam, alpha, dst_rows=np.arange(n), return_host=False)
        X = eng.read_factors(SIDE_USER, 0, n).astype(np.float64)
        D = ob.perturbations(X)                            # zero for the zero rows of the queries without entries
        eng.write_factors(SIDE_USER, ob.random_rows(n, k), n)
        eng.write_factors(SIDE_USER, X + D, 2 * n)
        eng.write_factors(SIDE_USER, X - D, 3 * n)
        _ladders[key] = (eng, lad, n)
    return _ladders[key]


@pytest.mark.parametrize("precision,case", LADDER, ids=LADDER_IDS)
def test_ladder(gpu, precision, case):
    k, alpha, lam = case
    eng, lad, n = ladder_state(gpu, precision, case)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.implicit_objective_plan(n) == objective_plan(eng.kp, 4 if precision == "f32" else 8, n, cu)
    tag = f"ladder {precision} k={k} (stride {eng.kp}) alpha={alpha:g} lam={lam:g}"
    check(tag + " solved rows", eng, queries(lad), np.arange(n), lam, alpha)
    check(tag + " random rows", eng, queries(lad), n + np.arange(n), lam, alpha)


@pytest.mark.parametrize("precision,case", LADDER, ids=LADDER_IDS)
def test_minimiser_on_the_device(gpu, precision, case):
    k, alpha, lam = case
    eng, lad, n = ladder_state(gpu, precision, case)
    f = [eng.implicit_objective(SIDE_USER, queries(lad), off + np.arange(n), lam, alpha, parts=True)["parts"].sum(axis=1)
         for off in (0, 2 * n, 3 * n)]
    rated = lad.degs > 0
    rise = np.minimum(f[1] - f[0], f[2] - f[0])
    i = int(np.argmin(np.where(rated, rise / np.maximum(np.abs(f[0]), 1e-300), np.inf)))
    print(f"\n[objective] minimiser {precision} k={k}: smallest rise f(x +- d) - f(x) = {rise[i]:.3e} at row {i} "
          f"(f = {f[0][i]:.6e}, {int(lad.degs[i])} entries)")
    assert (rise[rated] > 0).all(), np.nonzero(rated & ~(rise > 0))[0][:12]
    assert not rise[~rated].any()                          # x = 0 and no entries: f = 0 at all three


@pytest.mark.parametrize("precision,case", [LADDER[2], LADDER[3], LADDER[5], LADDER[6]],
                         ids=[LADDER_IDS[i] for i in (2, 3, 5, 6)])
def test_batch_independence(gpu, precision, case):
    k, alpha, lam = case
    eng, lad, n = ladder_state(gpu, precision, case)
    assert [int(lad.degs[r]) for r in ALONE_ROWS] == [1, 32, 33, 330, 1025, 4000, 0, 0]

    def parts(rows):
        rows = list(rows)
        return eng.implicit_objective(SIDE_USER, queries(lad, rows), np.asarray(rows), lam, alpha, parts=True)["parts"]

    whole = parts(range(n))
    for r in ALONE_ROWS:
        assert np.array_equal(bits(parts([r])[0]), bits(whole[r])), (r, int(lad.degs[r]))
    assert np.array_equal(bits(parts(range(n - 1, -1, -1))[::-1]), bits(whole))
    assert np.array_equal(bits(parts(range(n))), bits(whole))
    # the same row listed by several queries: each gets the bits of its own entries at that x
    twice = eng.implicit_objective(SIDE_USER, queries(lad, [40, 40, 7]), np.array([40, 40, 40]), lam, alpha, parts=True)
    assert np.array_equal(bits(twice["parts"][0]), bits(whole[40])) and np.array_equal(bits(twice["parts"][1]), bits(whole[40]))


# ---------------------------------------------------------------------------------------------------------------------
# 2: more queries than workgroups
# ---------------------------------------------------------------------------------------------------------------------
def test_more_queries_than_workgroups(gpu):
    """5,000 queries of 1..8 entries over 512 opposite rows at k = 64, reading 64 user rows in turn: the grid-stride
    loop reuses a workgroup's LDS for several queries, and the longest-first order differs from the order given."""
    k, nq, n_opp, n_x = 64, 5000, 512, 64
    rng = np.random.default_rng(21)
    degs = 1 + np.arange(nq) % 8
    ptr = np.zeros(nq + 1, np.int64)
    np.cumsum(degs, out=ptr[1:])
    qs = (ptr, rng.integers(0, n_opp, ptr[-1]).astype(np.int32), rng.integers(1, 6, ptr[-1]).astype(np.int16))
    eng = make_engine(gpu, "f32", k, rs.factors(n_opp, k), n_x)
    try:
        eng.write_factors(SIDE_USER, ob.random_rows(n_x, k))
        assert eng.implicit_objective_plan(nq)["workgroups"] < nq
        rows = np.arange(nq) % n_x
        got = check("5000 queries", eng, qs, rows, EDGE_LAM, EDGE_ALPHA)
        first = eng.implicit_objective(SIDE_USER, (ptr[:345], qs[1], qs[2]), rows[:344], EDGE_LAM, EDGE_ALPHA, parts=True)
        assert np.array_equal(bits(first["parts"]), bits(got["parts"][:344]))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3: every width next to a stride edge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,k", EDGES, ids=[f"{p}-k{k}" for p, k in EDGES])
def test_stride_edges(gpu, precision, k):
    lad = rs.width_ladder()
    n = len(lad.degs)
    eng = make_engine(gpu, precision, k, rs.factors(lad.n_opp, k), n)
    try:
        eng.write_factors(SIDE_USER, ob.random_rows(n, k))
        check(f"width {precision} k={k} (stride {eng.kp})", eng, queries(lad), np.arange(n), EDGE_LAM, EDGE_ALPHA)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4: special entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,k", [("f32", 10), ("f32", 64), ("f32", 128), ("f64", 64), ("f64", 65)])
def test_special_entries(gpu, precision, k):
    lad = rs.width_ladder()
    n = len(lad.degs)
    ptr, idx, rat = queries(lad)
    eng = make_engine(gpu, precision, k, rs.factors(lad.n_opp, k), n + 1)
    try:
        eng.write_factors(SIDE_USER, ob.random_rows(n, k))            # row n stays zero
        rows = np.arange(n)

        def parts(qs, rows=rows):
            return eng.implicit_objective(SIDE_USER, qs, rows, EDGE_LAM, EDGE_ALPHA, parts=True)["parts"]

        plain = parts((ptr, idx, rat))
        # entries of rating 0: alone they give exactly 0.0, after a query's entries they leave its bits, anywhere they
        # leave it within the bound of the restatement (which has them at s^2 - s^2 = 0 too)
        zeros = parts((ptr, idx, np.zeros_like(rat)))
        assert not zeros[:, 1].any() and np.array_equal(bits(zeros[:, [0, 2]]), bits(plain[:, [0, 2]]))
        rng = np.random.default_rng(4)
        ptr2, idx2, rat2 = [0], [], []
        for q in range(n):
            extra = rng.integers(0, lad.n_opp, 1 + q % 5)
            idx2 += list(idx[ptr[q]:ptr[q + 1]]) + list(extra)
            rat2 += list(rat[ptr[q]:ptr[q + 1]]) + [0] * len(extra)
            ptr2.append(len(idx2))
        appended = parts((np.asarray(ptr2, np.int64), np.asarray(idx2, np.int32), np.asarray(rat2, np.int16)))
        assert np.array_equal(bits(appended), bits(plain))
        check(f"zero ratings {precision} k={k}", eng, ob.with_zero_ratings(lad), rows, EDGE_LAM, EDGE_ALPHA)
        # a duplicated item counts twice
        rep = rs.repeat_ladder()
        rq = queries(rep)
        nr = len(rep.degs)
        assert nr <= n and rep.n_opp <= lad.n_opp
        got = check(f"repeats {precision} k={k}", eng, rq, np.arange(nr), EDGE_LAM, EDGE_ALPHA)
        X = eng.read_factors(SIDE_USER, 0, nr).astype(np.float64)
        Y = eng.read_factors(SIDE_MOVIE).astype(np.float64)
        once, bound = ob.parts(rs.counted_once(rep.side), X, Y, eng.gram_table(SIDE_MOVIE), EDGE_LAM, EDGE_ALPHA)
        dup = np.abs(once[:, 1] - ob.parts(rq, X, Y, eng.gram_table(SIDE_MOVIE), EDGE_LAM, EDGE_ALPHA)[0][:, 1]) > 0
        assert dup.any() and (np.abs(got["parts"][dup, 1] - once[dup, 1]) > ob.MUTANT_MARGIN * bound[dup, 1]).all()
        # a zero x row: {0, sum_{r > 0} (1 + alpha r), 0}; alpha = 10 makes every term and sum an exact integer
        zero_x = parts((ptr, idx, rat), np.full(n, n))
        want = np.array([float(np.sum(1.0 + EDGE_ALPHA * rat[ptr[q]:ptr[q + 1]].astype(np.float64))) for q in range(n)])
        assert not zero_x[:, [0, 2]].any() and np.array_equal(zero_x[:, 1], want)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5: training
# ---------------------------------------------------------------------------------------------------------------------
def loss_tolerance(app, alpha, precision):
    """The sum of the bounds of the call over all users, and in fp32 the table Gram's n u (sum_q |x|^T (|Y|^T |Y|) |x| +
    lambda tr(|Y|^T |Y|)) on top: G's own derived bound (n u |Y|^T |Y| per element) carried through x^T G x and tr."""
    eng = app.engine
    row_ptr, col, rat, row_offset, n_rows = app._implicit_csr(SIDE_USER)
    X = eng.read_factors(SIDE_USER).astype(np.float64)[row_offset:row_offset + n_rows]
    Y = eng.read_factors(SIDE_MOVIE).astype(np.float64)
    G = eng.gram_table(SIDE_MOVIE).astype(np.float64)
    lam = float(np.float32(app.ALS_LAMBDA))
    _, bound = ob.parts((row_ptr, col, rat), X, Y, G, lam, alpha)
    tol = float(bound.sum()) + (eng.k + 2) * ob.U * lam * float(np.trace(np.abs(G)))
    if precision == "f32":
        aG = np.abs(Y).T @ np.abs(Y)
        tol += len(Y) * 2.0 ** -24 * (float(np.einsum("qi,ij,qj->", np.abs(X), aG, np.abs(X))) + lam * float(np.trace(aG)))
    return tol


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_training(gpu, precision):
    t = ir.TRAIN
    _, (m, u, r) = ir.train_inputs()
    ds = gpu.Dataset.from_ratings(m, u, r)
    k, lam, alpha = t["k"], t["lam"], t["alpha"]
    app = gpu.ALSApp(1, k, lam, 4, precision=precision, seed=t["seed"]).setup(ds)
    prev = app.implicit_objective(alpha)["loss"]
    assert abs(prev - app.implicit_loss(alpha)) <= loss_tolerance(app, alpha, precision)
    worst = 0.0
    for h in range(t["halves"]):
        app.implicit_half(SIDE_MOVIE if h % 2 == 0 else SIDE_USER, alpha)
        got = app.implicit_objective(alpha)
        host = app.implicit_loss(alpha)
        tol = loss_tolerance(app, alpha, precision)
        worst = max(worst, abs(got["loss"] - host) / tol)
        print(f"\n[objective] training {precision} half {h}: device loss {got['loss']:.9f}, host loss {host:.9f}, "
              f"|difference| {abs(got['loss'] - host):.3e} = {abs(got['loss'] - host) / tol:.3e} of the tolerance {tol:.3e}")
        assert abs(got["loss"] - host) <= tol
        assert got["loss"] < prev
        prev = got["loss"]
    print(f"[objective] training {precision}: worst fraction of the tolerance {worst:.3e}")


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_implicit_fit(gpu, precision):
    t = ir.TRAIN
    _, (m, u, r) = ir.train_inputs()
    ds = gpu.Dataset.from_ratings(m, u, r)

    def fresh():
        return gpu.ALSApp(1, t["k"], t["lam"], 4, precision=precision, seed=t["seed"]).setup(ds)

    want = ob.train_losses(ds.init_user_factors(t["k"], t["seed"]))
    tol = ob.fit_stop(want, ob.FIT_STOP)
    losses = fresh().implicit_fit(t["alpha"], 3)
    print(f"\n[objective] fit {precision}: losses {losses}, the fp64 restatement's {want[:4]}")
    assert len(losses) == 4 and all(b < a for a, b in zip(losses, losses[1:]))
    stopped = fresh().implicit_fit(t["alpha"], ob.FIT_ITERATIONS, rel_tol=tol)
    assert len(stopped) == ob.FIT_STOP + 1 and stopped == losses[:ob.FIT_STOP + 1]
    assert fresh().implicit_fit(t["alpha"], 0) == losses[:1]


# ---------------------------------------------------------------------------------------------------------------------
# 6: the contract
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_untouched_tables(gpu):
    from cfk_amd import _lib
    L = _lib.lib()
    k, lam, alpha = 32, 0.2, 10.0
    lad, F, _ = ir.ladder_case(32, 10.0, 0.2)
    n_user_rows = 8
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, "f32")
        bare = gpu.ALSEngine(k, "f32")
        wide = gpu.ALSEngine(200, "f32")
    qp = np.array([0, 2, 3], np.int64)
    qi = np.array([5, 6, 7], np.int32)
    qr = np.array([1, 2, 3], np.int16)
    rows = np.array([1, 3], np.int64)
    parts = np.full((2, 3), 7.0)
    totals = np.full(4, 7.0)

    def p(a, ct):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))

    def raw(e, side=SIDE_USER, n=2, ptr=qp, idx=qi, rat=qr, rows=rows, lam=lam, alpha=alpha, parts=parts, totals=totals):
        st = L.als_implicit_objective(e._h, side, n, p(ptr, ctypes.c_int64), p(idx, ctypes.c_int32), p(rat, ctypes.c_int16),
                                      p(rows, ctypes.c_int64), ctypes.c_float(lam), ctypes.c_float(alpha),
                                      p(parts, ctypes.c_double), p(totals, ctypes.c_double))
        return st, L.als_last_error().decode()

    try:
        eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
        eng.write_factors(SIDE_MOVIE, F)
        st, msg = raw(eng)                                                      # this side's factors are not bound
        assert st == 5 and "side 1" in msg, msg
        st, msg = raw(bare)                                                     # no factors at all
        assert st == 5 and "side 0" in msg, msg
        eng.alloc_factors(SIDE_USER, n_user_rows)
        eng.write_factors(SIDE_USER, ob.random_rows(n_user_rows, k))
        tables = [eng.factors[s].cpu().numpy().copy() for s in (SIDE_MOVIE, SIDE_USER)]
        assert raw(eng)[0] == 0 and not (parts == 7.0).any() and not (totals == 7.0).any()    # the valid call
        good = parts.copy()
        parts.fill(7.0)
        totals.fill(7.0)
        INVALID = [
            ("bad side", dict(side=2), None),
            ("negative n_queries", dict(n=-1), None),
            ("NULL q_ptr", dict(ptr=None), None),
            ("NULL q_idx", dict(idx=None), None),
            ("NULL q_ratings", dict(rat=None), None),
            ("NULL rows", dict(rows=None), "rows"),
            ("NULL totals", dict(totals=None), "totals"),
            ("decreasing q_ptr", dict(ptr=np.array([0, 2, 1], np.int64)), "query 1"),
            ("index past the table", dict(idx=np.array([5, 6, lad.n_opp], np.int32)), "query 1"),
            ("negative index", dict(idx=np.array([5, -1, 7], np.int32)), "query 0"),
            ("2^31 entries", dict(ptr=np.array([0, 2, 1 << 31], np.int64)), "2^31"),
            ("row past the table", dict(rows=np.array([1, n_user_rows], np.int64)),
             f"rows[1] = {n_user_rows} of query 1 is outside [0, {n_user_rows})"),
            ("negative row", dict(rows=np.array([-1, 2], np.int64)), "rows[0] = -1 of query 0"),
            ("negative rating", dict(rat=np.array([1, 2, -1], np.int16)), "rating -1 of query 1 is negative"),
            ("negative rating in query 0", dict(rat=np.array([1, -3, 2], np.int16)), "rating -3 of query 0 is negative"),
            ("lambda 0", dict(lam=0.0), "lambda must be positive and finite"),
            ("lambda negative", dict(lam=-0.05), "lambda must be positive and finite"),
            ("lambda nan", dict(lam=float("nan")), "lambda must be positive and finite"),
            ("lambda inf", dict(lam=float("inf")), "lambda must be positive and finite"),
            ("alpha 0", dict(alpha=0.0), "alpha must be positive and finite"),
            ("alpha negative", dict(alpha=-1.0), "alpha must be positive and finite"),
            ("alpha nan", dict(alpha=float("nan")), "alpha must be positive and finite"),
            ("alpha inf", dict(alpha=float("inf")), "alpha must be positive and finite"),
        ]
        for name, kw, needle in INVALID:
            st, msg = raw(eng, **kw)
            assert st == 1 and msg.startswith("als_implicit_objective:") or name == "bad side" and st == 1, (name, st, msg)
            assert needle is None or needle in msg, (name, msg)
            assert (parts == 7.0).all() and (totals == 7.0).all(), name         # a failed call writes nothing
        # a repeated row is allowed, and a rebased q_ptr gives the same bits
        assert raw(eng, rows=np.array([3, 3], np.int64))[0] == 0
        st, _ = raw(eng, ptr=qp + 3, idx=np.concatenate([np.array([9, 9, 9], np.int32), qi]),
                    rat=np.concatenate([np.array([5, 5, -5], np.int16), qr]))
        assert st == 0 and np.array_equal(bits(parts), bits(good))
        # host_parts NULL: the totals alone
        t2 = np.full(4, 7.0)
        assert raw(eng, parts=None, totals=t2)[0] == 0 and np.array_equal(bits(t2), bits(totals))
        # nothing to do: four zeros, no pointer read
        assert raw(eng, n=0, ptr=None, idx=None, rat=None, rows=None, parts=None, totals=t2)[0] == 0 and not t2.any()
        # an unsupported width
        wide.alloc_factors(SIDE_MOVIE, 16)
        wide.alloc_factors(SIDE_USER, 16)
        st, msg = raw(wide)
        assert st == 2 and "128" in msg, msg
        info = (ctypes.c_int64 * 4)()
        assert L.als_implicit_objective_plan(wide._h, 2, info) == 2 and L.als_implicit_objective_plan(eng._h, -1, info) == 1
        assert L.als_implicit_objective_plan(eng._h, 2, None) == 1
        assert L.als_implicit_objective_plan(eng._h, 2, info) == 0 and list(info) == [256, 2, 0, 8 * (32 + 16)]
        # the Python wrapper raises the same statuses
        with pytest.raises(gpu.ALSError) as e:
            eng.implicit_objective(SIDE_USER, (qp, qi, np.array([1, 2, -1], np.int16)), rows, lam, alpha)
        assert e.value.status == 1 and "query 1" in str(e.value)
        assert eng.implicit_objective(SIDE_USER, (np.zeros(1, np.int64), [], []), [], lam, alpha, parts=True)["parts"].shape == (0, 3)
        # both factor tables are bitwise unchanged by all of the above
        for s, before in zip((SIDE_MOVIE, SIDE_USER), tables):
            assert np.array_equal(bits(eng.factors[s].cpu().numpy()), bits(before))
    finally:
        for e in (eng, bare, wide):
            e.close()


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
                rows = list(range(0, n // 2, 9))                         # rows of the chunk that is solved already
                got = eng.implicit_objective(SIDE_USER, queries(lad, rows), np.asarray(rows), 0.1, 10.0, parts=True)
                assert got["parts"].shape == (len(rows), 3) and got["parts"].all() and got["ridge_opp"] > 0
            eng.solve_half_chunk(SIDE_USER, lam, 1)
            out.append(eng.read_factors(SIDE_USER, 0, n))
            assert eng.integrity_status() == [0, 0, 0, 0]
        finally:
            eng.close()
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.any(out[0][n // 2:] != 0)
