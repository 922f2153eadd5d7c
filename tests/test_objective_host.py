"""CPU side of als_implicit_objective (no kernel launch): the numpy restatement of objective_ref.py against the dense loss
and against the closed form at the minimiser, the distance of every mutant from every row it changes, the launch plan and
the `rows` check under the sanitizers, and the bindings.

tests/plan/objective_plan_check.cpp and tests/host/objective_args_check.cpp are compiled by the host C++ compiler under
AddressSanitizer + UBSan and run as programs of their own, as tests/test_similar_host.py runs its two: nothing is
preloaded and no Python runs in the sanitizer run.

Measured here (every figure is re-measured by the tests below): sum_q f_q + lambda tr(G) is within 1.4e-16 of the dense
loss; f at the oracle's solution is within 0.021 of the summed bounds of c - b^T x and grows by d^T A d to 0.017 of the
tolerance; the nearest mutant over all ladder cases, both x sets and the zero-rating inputs is 5.7e3 bounds away (fp64
k = 128), so every (k, alpha, lambda) of implicit_ref's ladder, and k = 65 at the fp64 parameters, is used on the GPU as
it stands: no case had to be replaced.
"""
import json
import os
import re

import numpy as np
import pytest

import implicit_ref as ir
import objective_ref as ob
from conftest import ROOT
from test_plan_host import CSRC
from test_similar_host import _sanitized

LADDER = tuple(ob.LADDER_F32) + tuple(ob.LADDER_F64) + ((65, 40.0, 0.05),)
OBJECTIVE_WG_PER_CU, OBJECTIVE_RED_SLOTS = 5, 16


def objective_plan(kp: int, elem_bytes: int, n_queries: int, cu_count: int) -> dict:
    """cfk::objective_plan restated: 256 threads, 5 workgroups per compute unit but never more than the queries, x and
    the waves' sums as doubles."""
    return {"threads": 256, "workgroups": max(1, min(n_queries, OBJECTIVE_WG_PER_CU * max(1, cu_count))),
            "lds_bytes": 8 * (kp + OBJECTIVE_RED_SLOTS)}


def group_lanes(kp: int, elem_bytes: int) -> int:
    lanes = 1
    while lanes * 16 < kp * elem_bytes:
        lanes *= 2
    return lanes


def user_queries(R):
    return ir.dense_to_csr(R)


def test_extended_precision_is_available():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63      # the reference sums carry 11 bits more than the bounds' unit


# ---------------------------------------------------------------------------------------------------------------------
# the sum of f is the loss over the grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factors", ["random", "trained"])
def test_sum_of_f_plus_ridge_is_the_dense_loss(factors):
    t = ir.TRAIN
    R, _ = ir.train_inputs()
    rng = np.random.default_rng(9)
    U, M = rng.standard_normal((t["n_users"], t["k"])) / 3, rng.standard_normal((t["n_movies"], t["k"])) / 3
    if factors == "trained":
        U, M = ir.train(R, np.abs(U), t["lam"], t["alpha"], t["halves"])[-1]
    G = M.T @ M
    p, _ = ob.parts(user_queries(R), U, M, G, t["lam"], t["alpha"])
    total = float(p.sum() + float(np.float32(t["lam"])) * np.trace(G))
    want = ir.loss(U, M, R, t["lam"], t["alpha"])
    print(f"\n[objective] {factors}: sum f + lambda tr G = {total:.12f}, dense loss {want:.12f}, "
          f"relative {abs(total - want) / want:.2e}")
    assert abs(total - want) <= 1e-12 * want
    # and from the movie side: the same loss
    pm, _ = ob.parts(user_queries(R.T), M, U, U.T @ U, t["lam"], t["alpha"])
    assert abs(float(pm.sum() + float(np.float32(t["lam"])) * np.trace(U.T @ U)) - want) <= 1e-12 * want


# ---------------------------------------------------------------------------------------------------------------------
# the ladder: the closed form at the minimiser, and f grows by d^T A d around it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LADDER, ids=lambda c: "k%d-a%g-l%g" % c)
def test_f_at_the_solution_is_the_closed_form(case):
    k, alpha, lam = case
    lad, F, ref64 = ir.ladder_case(*case)
    G = F.T @ F
    p, b = ob.parts(lad.side, ref64, F, G, lam, alpha)
    want = ob.closed_form(lad.side, ref64, F, alpha)
    frac = np.abs(p.sum(axis=1) - want) / np.maximum(b.sum(axis=1), np.finfo(float).tiny)
    rated = lad.degs > 0
    print(f"\n[objective] closed form k={k} alpha={alpha:g} lam={lam:g}: worst |f - (c - b.x)| / bound = "
          f"{frac[rated].max():.3e} (row {int(np.argmax(np.where(rated, frac, -1)))})")
    assert (frac[rated] <= 1).all()
    assert not p[~rated].any() and not want[~rated].any()


@pytest.mark.parametrize("case", LADDER, ids=lambda c: "k%d-a%g-l%g" % c)
def test_f_grows_by_the_quadratic_form_around_the_solution(case):
    k, alpha, lam = case
    lad, F, ref64 = ir.ladder_case(*case)
    G = F.T @ F
    D = ob.perturbations(ref64)
    p0, b0 = ob.parts(lad.side, ref64, F, G, lam, alpha)
    p1, b1 = ob.parts(lad.side, ref64 + D, F, G, lam, alpha)
    worst = 0.0
    for q in np.nonzero(lad.degs > 0)[0]:
        A, b = ob.system(lad.side, q, F, G, lam, alpha)
        d, x = D[q], ref64[q]
        # f(x + d) - f(x) = d^T A d + 2 d^T (A x - b) exactly; the second term is the solver's residual
        want = d @ A @ d + 2 * d @ (A @ x - b)
        tol = b0[q].sum() + b1[q].sum() + (2 * k + 4) * ob.U * (np.abs(d) @ np.abs(A) @ np.abs(d) +
                                                              2 * np.abs(d) @ (np.abs(A) @ np.abs(x) + np.abs(b)))
        got = p1[q].sum() - p0[q].sum()
        worst = max(worst, abs(got - want) / tol)
        assert abs(got - want) <= tol and got > 0, (int(q), got, want, tol)
    print(f"\n[objective] growth k={k}: worst |df - d^T A d| / tolerance = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# every mutant is far from every row it changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LADDER, ids=lambda c: "k%d-a%g-l%g" % c)
def test_mutants_are_far_from_every_row_they_change(case):
    k, alpha, lam = case
    lad, F, ref64 = ir.ladder_case(*case)
    G = F.T @ F
    n = len(lad.degs)
    nearest = np.inf
    for name, queries, X in (("solved", lad.side, ref64), ("random", lad.side, ob.random_rows(n, k)),
                             ("zero ratings", ob.with_zero_ratings(lad), ob.random_rows(n, k))):
        for m, (rows, margin) in ob.mutant_margins(queries, X, F, G, lam, alpha).items():
            if m == "p_one_for_zero":
                assert (rows > 0) == (name == "zero ratings"), (name, rows)
            else:
                assert rows > 0, (name, m)
            nearest = min(nearest, margin)
            assert margin >= ob.MUTANT_MARGIN, (name, m, rows, margin)
    print(f"\n[objective] mutants k={k} alpha={alpha:g} lam={lam:g}: nearest {nearest:.3e} bounds")


@pytest.mark.parametrize("k", [15, 64, 128])
def test_mutants_are_far_on_the_width_ladder(k):
    """The inputs of the GPU module's stride-edge and special-entry cases: the width ladder at random rows."""
    import rowshapes as rs
    lad = rs.width_ladder()
    F = rs.factors(lad.n_opp, k)
    X = ob.random_rows(len(lad.degs), k)
    for name, queries in (("plain", lad.side), ("zero ratings", ob.with_zero_ratings(lad))):
        for m, (rows, margin) in ob.mutant_margins(queries, X, F, F.T @ F, 0.1, 10.0).items():
            assert (rows > 0) or (m == "p_one_for_zero" and name == "plain"), (name, m)
            assert margin >= ob.MUTANT_MARGIN, (name, m, rows, margin)


# ---------------------------------------------------------------------------------------------------------------------
# the stopping rule of ALSApp.implicit_fit
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_stop_of_the_restatement(cfk):
    t = ir.TRAIN
    _, (m, u, r) = ir.train_inputs()
    ds = cfk.Dataset.from_ratings(m, u, r)
    losses = ob.train_losses(ds.init_user_factors(t["k"], t["seed"]))
    assert len(losses) == ob.FIT_ITERATIONS + 1 and all(b < a for a, b in zip(losses, losses[1:]))
    tol = ob.fit_stop(losses, ob.FIT_STOP)
    drops = [(a - b) / a for a, b in zip(losses, losses[1:])]
    print(f"\n[objective] restatement losses {losses}, relative drops {drops}, rel_tol {tol:.3e}")
    # the stopping iteration is a factor of at least 1.5 away from the drops on either side: fp32 training moves the
    # drops by far less
    assert drops[ob.FIT_STOP - 2] >= 1.5 * tol and drops[ob.FIT_STOP - 1] * 1.5 <= tol


# ---------------------------------------------------------------------------------------------------------------------
# the plan and the argument check under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_sweep_and_python_restatement(tmp_path_factory):
    out = json.loads(_sanitized(tmp_path_factory, "objective_plan_check",
                                [os.path.join(ROOT, "tests", "plan", "objective_plan_check.cpp"),
                                 os.path.join(CSRC, "als_plan.cpp")], [CSRC]))
    assert out["failed"] == {}
    assert out["cases"] == 11 * (70 + 18 + 11) * 3 == len(out["plans"])
    for key, (threads, grid, lds, lanes) in out["plans"].items():
        kp, elem, n, cu = map(int, key.split("/"))
        assert {"threads": threads, "workgroups": grid, "lds_bytes": lds} == objective_plan(kp, elem, n, cu), key
        assert lanes == group_lanes(kp, elem), key
    assert [group_lanes(kp, 8) for kp in (16, 80, 96, 112, 128)] == [8, 64, 64, 64, 64]
    assert [group_lanes(kp, 4) for kp in (16, 32, 64, 128)] == [4, 8, 16, 32]


ARG_CASES = {
    "ok": "", "ok_repeated_row": "", "ok_last_row_of_a_large_table": "", "ok_no_queries": "",
    "negative": "als_implicit_objective: rows[1] = -1 of query 1 is outside [0, 7)",
    "at_limit": "als_implicit_objective: rows[2] = 7 of query 2 is outside [0, 7)",
    "beyond_int32": "als_implicit_objective: rows[1] = 8589934592 of query 1 is outside [0, 7)",
    "first_fault_is_reported": "als_implicit_objective: rows[0] = 8 of query 0 is outside [0, 7)",
    "empty_table": "als_implicit_objective: rows[0] = 0 of query 0 is outside [0, 0)",
}


def test_rows_check(tmp_path_factory):
    out = _sanitized(tmp_path_factory, "objective_args_check",
                     [os.path.join(ROOT, "tests", "host", "objective_args_check.cpp"), os.path.join(CSRC, "als_args.cpp"),
                      os.path.join(CSRC, "als_error.cpp")], [CSRC, os.path.join(ROOT, "include")])
    got = {c["case"]: (c["status"], c["message"]) for c in map(json.loads, out.splitlines())}
    assert got == {name: (1 if msg else 0, msg) for name, msg in ARG_CASES.items()}


# ---------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_headers_declare_and_python_binds_the_calls(cfk):
    from cfk_amd import _lib
    als_h = open(os.path.join(ROOT, "include", "als.h")).read()
    assert re.search(r"^int als_implicit_objective\(als_engine\* e, int side, int64_t n_queries, const int64_t\* q_ptr, "
                     r"const int32_t\* q_idx,\n\s+const int16_t\* q_ratings, const int64_t\* rows, float lambda, float "
                     r"alpha, double\* host_parts,\n\s+double totals\[4\]\);", als_h, flags=re.M)
    assert re.search(r"^int als_implicit_objective_plan\(const als_engine\* e, int64_t n_queries, int64_t info\[4\]\);",
                     als_h, flags=re.M)
    assert "#define ALS_ABI_VERSION 3" in als_h                        # purely additive
    sigs = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sigs["als_implicit_objective"]) == 11 and len(sigs["als_implicit_objective_plan"]) == 3
    L = _lib.lib()
    assert L.als_implicit_objective.argtypes == sigs["als_implicit_objective"]
    assert L.als_implicit_objective_plan.argtypes == sigs["als_implicit_objective_plan"]
    assert L.als_abi_version() == 3
    assert callable(cfk.ALSEngine.implicit_objective) and callable(cfk.ALSEngine.implicit_objective_plan)
    assert callable(cfk.ALSApp.implicit_objective) and callable(cfk.ALSApp.implicit_fit)
