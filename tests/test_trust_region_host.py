"""The trust-region cases (tests/trust_region_cases.py) certified WITHOUT a device: for every case the float64 twin, the
longdouble twin (tests/trust_region_reference.py) and the oracle agree on status, iteration count, accept pattern, convergence
flags and call counts; the twin's branch labels contain the branches the case names; and every comparison that decides a
branch is away from its threshold.  tests/test_v_gpu_trust_region.py then holds every loop driver of the library to these
certified values.  `pytest -s` prints the case table (TRCASE), the coverage table (TRCOVER) and the searches (TRSEARCH).

Margins.  The trajectory tests allow rtol = 1e-8 between device and oracle for rho and delta (tests/test_a_gpu_contract.py), so
a comparison `value <op> threshold` certifies a branch only if |value - threshold| >= 1e-5 max(|value|, |threshold|) -- 1e3
times that -- in BOTH precisions.  The exception is a comparison that is exact by construction: value == threshold in both
precisions (the scripted integer cases: rho == 0.25, rho == 0.75; exact zeros: dx = 0 against x_tol = 0, a zero gradient, a
clip onto the bound).  For the scripted cases (Case.exact) the oracle's counts, flags, accept pattern and delta trace are also
asserted identical in every summation mode of the oracle, and for the Dogleg ones, whose Gauss-Newton solve on [I; 0] is exact,
rho itself is the twin's bit for bit.  cc of Dogleg's case 3 is compared against 0 on the scale of its two terms.

Toy cases are certified twice: with the direct solve (the dense QR() / Cholesky() drivers) and with the LSMR solve (the twin
calls tests/lsmr_reference.py; the drivers that iterate), where the inner iteration counts must agree as well.  The
index-spread cases are certified with LSMR, the only solver a general sparse handle iterates with.

cc <= 0 in case 3 (test_cc_nonpositive_search): with an exact Gauss-Newton step Cauchy-Schwarz gives cc >= 0.  Searched: the
model r = A tanh(x) - b on 4 x 2 ... 12 x 8 matrices with entries N(0, 1), columns scaled by 10^U(-2, 2), x0 ~ U(-1, 1)^n,
delta in {0.01, 0.1, 0.5, 1, 2} x wnorm(x0), 4 iterations each, 60 seeds, with the direct and with the LSMR solve: 600 runs.
The direct solve never takes the branch.  The LSMR solve (tolerance 1e-6 relative, so dgn is inexact) is reported; if it takes
the branch with |cc| beyond the margin the case belongs in the table.

The CPU copy of the LM loop in rowshard.lm_lsmr runs here on its numpy backend at world 1 through every LM case without bounds
(it takes none).  loops.py (optimize_operator_level) makes device calls for every array operation: it is a driver of
tests/test_v_gpu_trust_region.py.

Planted errors (test_planted_errors): five mistakes planted in the twin, each of which must change what a certified case
expects -- the cases discriminate.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import trust_region_cases as TC
import trust_region_reference as R

LD = np.longdouble
NAMES = list(TC.cases())
MARGIN = 1e-5
ORACLE_SUM_MODES = (0, 1, 2, 3, 4, 5, 6)


def _away(v, t, scale=None):
    v, t = LD(v), LD(t)
    if np.isnan(v) or np.isnan(t):
        return True                       # (a NaN decides nothing by being close to a threshold)
    if v == t:
        return True                       # exact by construction; the caller checks it is so in both precisions
    if np.isinf(v) or np.isinf(t):
        return True
    s = max(abs(v), abs(t)) if scale is None else LD(scale)
    return abs(v - t) >= MARGIN * s


def check_margins(run, label):
    """Every recorded comparison of every iteration; returns the set of (iteration, name) that are exact ties."""
    ties = set()
    for k, rec in enumerate(run.its):
        for name, mg in rec["margins"].items():
            if name == "clamp":
                cs, lo, hi = mg
                for i, c in enumerate(cs):
                    assert _away(c, lo) and _away(c, hi), (label, k, name, i, float(c), float(lo), float(hi))
                continue
            v, t = mg
            if name == "cc":
                assert _away(v, 0, scale=abs(t)), (label, k, name, float(v), float(t))
                continue
            assert _away(v, t), (label, k, name, float(v), float(t))
            if np.isfinite(LD(v)) and LD(v) == LD(t):       # (inf against inf is float64 overflow, not a tie of two values)
                ties.add((k, name))
    return ties


def trace_of(run):
    return dict(delta=[float(r["delta"]) for r in run.its], rho=[float(r["rho"]) for r in run.its],
                gnorm=[float(r["maxabs_gr"]) for r in run.its], inner=[int(r["inner"]) for r in run.its],
                accept=[int(r["accepted"]) for r in run.its])


def differs(run, z, kdim):
    """Does `run` (a twin run with an error planted) miss what the device tier asserts for the certified z?  The same
    assertions: summary, accept pattern, branch-pure deltas bit for bit, continuous values inside the bounds of
    trust_region_cases.trajectory_pieces."""
    if TC.summary(run) != TC.summary(z.f64):
        return True
    a, b = trace_of(run), trace_of(z.f64)
    if a["accept"] != b["accept"]:
        return True
    for k, rec in enumerate(z.f64.its):         # a branch-pure delta: bit for bit from the delta before it
        if k and rec["pure_delta"] and a["delta"][k] != R.pure_delta(rec["pure_op"], a["delta"][k - 1]):
            return True
    mine = dict(rho=a["rho"], ssr=[float(r["ssr"]) for r in run.its], gnorm=a["gnorm"], delta=a["delta"],
                x=[np.asarray(r["x"], dtype=np.float64) for r in run.its])
    for i, what, hp, cond, bound in TC.trajectory_pieces(z.f64, z.ld, z.oracle.trace, kdim):
        if what != "x" and np.isnan(LD(hp)):
            continue
        if TC.piece_err(what, mine[what][i], hp) > bound:
            return True
    return False


def _agree(z, label, inner):
    s = TC.summary(z.f64)
    assert s == TC.summary(z.ld) == TC.summary(z.oracle), (label, s, TC.summary(z.ld), TC.summary(z.oracle))
    acc = [int(r["accepted"]) for r in z.ld.its]
    assert z.accept == acc == [int(v) for v in z.oracle.trace["accept"]], label
    if inner:
        assert [r["inner"] for r in z.f64.its] == [r["inner"] for r in z.ld.its] == [int(v) for v in z.oracle.trace["inner"]], label
    if z.f64.status != R.OK:
        return
    # the float64 twin and the oracle are two float64 statements of the same loop.  rho is a quotient of two differences of
    # sums of squares: its rounding error is that of ssr, 2^-53 m ssr, over pred_red -- large once the steps are small
    for k, rec in enumerate(z.f64.its):
        for key, val in (("delta", rec["delta"]), ("rho", rec["rho"]), ("gnorm", rec["maxabs_gr"]), ("ssr", rec["ssr"])):
            o = float(z.oracle.trace[key][k])
            if np.isnan(o) or np.isnan(float(val)):
                assert np.isnan(o) and np.isnan(float(val)), (label, k, key)
                continue
            tol = 1e-9 * max(abs(o), abs(float(val)))
            if key in ("rho", "delta") and float(rec["pred_red"]) > 0:
                tol *= max(1.0, float(rec["ssr"]) / float(rec["pred_red"]))
            if key == "gnorm":      # (J'f cancels as the fit converges: its error stays that of the first gradient's terms)
                tol += 1e-12 * float(z.f64.its[0]["maxabs_gr"])
            assert abs(o - float(val)) <= tol, (label, k, key, o, float(val))


@pytest.mark.parametrize("solver", ["direct", "lsmr"])
@pytest.mark.parametrize("name", NAMES)
def test_case_is_certified(name, solver):
    z = TC.certify(name, solver)
    c = z.case
    label = "%s/%s" % (name, solver)
    print("TRCASE %-32s %-6s status %d iter %2d accept %s flags %d%d%d f %d g %d | %s"
          % (name, solver, z.f64.status, z.f64.iterations, "".join(map(str, z.accept)) or "-", z.f64.x_converged,
             z.f64.f_converged, z.f64.g_converged, z.f64.f_calls, z.f64.g_calls, " ".join(sorted(c.branches))))
    _agree(z, label, inner=solver == "lsmr")
    # the problem was called as often as the loop says it was
    assert (z.f64.f_script_calls, z.f64.g_script_calls) == (z.f64.f_calls, z.f64.g_calls)
    assert (z.oracle.f_script_calls, z.oracle.g_script_calls) == (z.oracle.f_calls, z.oracle.g_calls)
    # the branches the case is there for
    assert c.branches <= z.labels, (label, sorted(c.branches - z.labels))
    # margins, and ties only where both precisions tie
    t64, tld = check_margins(z.f64, label + "/f64"), check_margins(z.ld, label + "/ld")
    assert t64 == tld, (label, sorted(t64 ^ tld))
    if t64 - {(k, n) for k, n in t64 if n in ("x_tol", "g_tol", "f_tol", "case1")}:
        assert c.exact, (label, sorted(t64))        # a tie on rho or delta is a scripted case's business
    for k, rec in enumerate(z.f64.its):             # bounded cases: every iterate inside the box
        lo, hi = c.opts["lower"], c.opts["upper"]
        assert lo is None or np.all(rec["x"] >= lo), (label, k)
        assert hi is None or np.all(rec["x"] <= hi), (label, k)


@pytest.mark.parametrize("name", [n for n in NAMES if TC.cases()[n].exact])
def test_exact_case_in_every_summation_mode(name):
    from oracle import oracle as O
    z = TC.certify(name)
    c = z.case
    want = (TC.summary(z.oracle), list(z.oracle.trace["accept"]), list(z.oracle.trace["delta"]))
    try:
        for mode in ORACLE_SUM_MODES:
            O.set_sum_mode(mode)
            for solver in (O.QR, O.CHOLESKY):
                if solver == O.CHOLESKY and "nonfinite" in name:
                    continue                 # (a NaN Jacobian is refused by the factorisation: another status, another test)
                r = TC.oracle(c, solver)
                got = (TC.summary(r), list(r.trace["accept"]), list(r.trace["delta"]))
                if c.kind == "dogleg" and "clamp" not in name:
                    assert got == want, (name, mode, solver)
                    assert all(float(a) == float(rec["rho"]) or (np.isnan(a) and np.isnan(float(rec["rho"])))
                               for a, rec in zip(r.trace["rho"], z.f64.its)), (name, mode)
                else:                        # LM's damped solve rounds: delta is exact only where it is a pure function
                    assert got[:2] == want[:2], (name, mode, solver)
                    for k, rec in enumerate(z.f64.its):
                        a, b = float(r.trace["delta"][k]), float(rec["delta"])
                        assert abs(a - b) <= 1e-9 * abs(b), (name, mode, k, a, b)
                        if k and rec["pure_delta"]:
                            assert a == R.pure_delta(rec["pure_op"], float(r.trace["delta"][k - 1])), (name, mode, k)
    finally:
        O.set_sum_mode(0)


SPREAD = [(n, kind, bounded) for n in TC.SPREAD_N for kind in ("lm", "dogleg") for bounded in (True, False)]


@pytest.mark.parametrize("n,kind,bounded", SPREAD)
def test_spread_is_certified(n, kind, bounded):
    z = TC.certify_spread(n, kind, bounded)
    p = z.problem
    label = "spread/%d/%s/%s" % (n, kind, "bounded" if bounded else "free")
    _agree(z, label, inner=True)
    assert check_margins(z.f64, label) == check_margins(z.ld, label)
    e_ref = TC.rel_err(z.oracle.minimizer, z.ld.x)
    print("TRCASE %-28s iter %d accept %s inner %s e_ref %.2e" % (label, z.f64.iterations, "".join(map(str, z.accept)),
                                                                 [r["inner"] for r in z.f64.its], e_ref))
    assert e_ref <= 1e-6                                     # beyond that a ratio of two errors says nothing
    assert np.array_equal(np.diff(np.sort(np.abs(p.vals[:, 0]))) > 0, np.ones(n - 1, dtype=bool))    # no two columns alike
    if not bounded:
        assert all(len(r.get("zeroed", ())) == 0 and len(r["clipped"]) == 0 for r in z.f64.its)
        return
    assert np.all(p.x0 >= p.lower) and np.all(p.x0 <= p.upper)                  # the start is feasible
    for run, x in ((z.f64, z.f64.x), (z.ld, z.ld.x), (z.oracle, z.oracle.minimizer)):
        at = np.where(np.isfinite(p.upper[p.at]), p.upper[p.at], p.lower[p.at])
        assert np.array_equal(np.asarray(x, dtype=np.float64)[p.at], at), label   # every bounded component ends ON its bound
    clipped, zeroed, largest = set(), set(), 0
    for run in (z.f64, z.ld):
        for rec in run.its:
            assert np.all(rec["x"] >= p.lower) and np.all(rec["x"] <= p.upper)
            clipped.update(rec["clipped"].tolist())
            zs = rec.get("zeroed")
            if zs is None or not len(zs):
                continue
            zeroed.update(zs.tolist())
            # the largest |g_i| of the whole vector is a projected one: a missed projection changes maxabs_gr itself
            assert float(rec["maxabs_gr"]) <= (1 - 1e3 * MARGIN) * float(rec["maxabs_g_raw"]), (label, float(rec["maxabs_gr"]))
            largest += 1
    assert clipped == set(p.at.tolist()) == zeroed, (label, sorted(clipped), sorted(zeroed))
    assert largest >= 2


def test_coverage():
    """Every branch the tier was asked for has a certified case that names it, or is listed as not reached."""
    have = {"lm": {}, "dogleg": {}}
    for name in NAMES:
        z = TC.certify(name)
        for lab in z.case.branches & z.labels:
            have[z.case.kind].setdefault(lab, []).append(name)
    unreached = []
    for kind, table in TC.BRANCHES.items():
        for what, lab in table.items():
            if lab is None:
                unreached.append((kind, what))
                print("TRCOVER %-7s %-44s NOT REACHED (tests/trust_region_cases.py)" % (kind, what))
                continue
            names = have[kind].get(lab, [])
            print("TRCOVER %-7s %-44s %s" % (kind, what, ", ".join(names)))
            assert names, (kind, what, lab)
    assert sorted(unreached) == sorted([("lm", "colsumabs2 clamped at MAX_DIAGONAL * mean"), ("dogleg", "beta for cc <= 0")])
    # decrease_factor 2, 4, ... 2048 down to the floor at iteration 11 from delta = 10, as the oracle was seen to do
    z = TC.certify("lm_reject_to_floor")
    assert [i for i, r in enumerate(z.f64.its, 1) if "delta_floor" in r["labels"]][0] == 11
    assert [float(r["delta"]) for r in z.f64.its[:3]] == [5.0, 1.25, 0.15625] and float(z.f64.its[-1]["delta"]) == 1e-16
    z = TC.certify("dogleg_halve_to_floor")
    assert float(z.f64.its[-1]["delta"]) == 1e-16 and len(z.f64.its) <= 60 and z.f64.g_calls == 1
    z = TC.certify("lm_delta_cap")
    assert float(z.f64.its[0]["delta"]) == 1e16
    # the index-spread cases put an active bound on every index they are there for
    assert set(TC.spread(16385).at.tolist()) == {0, 255, 256, 1023, 1024, 2047, 2048, 15359, 15360, 16384}


def test_cc_nonpositive_search():
    """The bounded search of the module docstring."""
    found = {"direct": 0, "lsmr": 0}
    beyond = []
    runs = 0
    for seed in range(60):
        rng = np.random.default_rng(seed)
        m, n = int(rng.integers(4, 13)), int(rng.integers(2, 9))
        m = max(m, n + 1)
        A = rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-2, 2, n)
        b = A @ np.tanh(rng.uniform(-1, 1, n)) + 0.05 * rng.standard_normal(m)
        x0 = rng.uniform(-1, 1, n)
        for scale in (0.01, 0.1, 0.5, 1.0, 2.0):
            for solver in ("direct", "lsmr"):
                c = TC.Case("search", "dogleg", lambda A=A, b=b: TC.Model(A=A, b=b), set(), x0=x0, iterations=4, delta=scale,
                            **TC.ZERO)
                c.m, c.n = m, n
                r = TC.twin(c, solver=solver)
                runs += 1
                for rec in r.its:
                    if "beta_cc_nonpositive" in rec["labels"]:
                        found[solver] += 1
                        cc, a2 = rec["margins"]["cc"]
                        if abs(cc) >= MARGIN * abs(a2):
                            beyond.append((seed, scale, solver, float(cc), float(a2)))
    print("TRSEARCH cc <= 0: %d runs, iterations on the branch %s, beyond the margin %s" % (runs, found, beyond[:5]))
    assert runs == 600
    assert found["direct"] == 0
    assert not beyond, beyond[:5]       # a certifiable case: it belongs in tests/trust_region_cases.py


PLANTED = {
    "projection_skipped_from_1024": lambda: [(TC.certify_spread(n, k), TC.spread(n).twin(k, plant="projection_skipped_from_1024"))
                                             for n in (1025, 16385) for k in ("lm", "dogleg")],
    "dogleg_strictness_swapped": lambda: [(TC.certify(n), TC.twin(TC.cases()[n], plant="dogleg_strictness_swapped"))
                                          for n in ("dogleg_rho_eq_quarter", "dogleg_rho_eq_three_quarters")],
    "decrease_factor_not_reset": lambda: [(TC.certify(n), TC.twin(TC.cases()[n], plant="decrease_factor_not_reset"))
                                          for n in ("lm_decrease_factor_reset",)],
    "f_converged_on_rejected_step": lambda: [(TC.certify(n), TC.twin(TC.cases()[n], plant="f_converged_on_rejected_step"))
                                             for n in ("lm_f_on_rejected_step", "dogleg_f_on_rejected_step")],
    "dogleg_clamp_relative": lambda: [(TC.certify(n), TC.twin(TC.cases()[n], plant="dogleg_clamp_relative"))
                                      for n in ("dogleg_clamp_absolute",)],
}


@pytest.mark.parametrize("plant", list(R.PLANTS))
def test_planted_errors(plant):
    pairs = PLANTED[plant]()
    assert pairs
    for z, run in pairs:
        kdim = z.problem.m if hasattr(z, "problem") else max(z.case.m, z.case.n)
        assert differs(run, z, kdim), plant
        assert not differs(z.f64, z, kdim)
    if plant == "projection_skipped_from_1024":        # ... and the sizes below the first skipped index cannot see it
        z = TC.certify_spread(1024, "lm")
        assert not differs(TC.spread(1024).twin("lm", plant=plant), z, z.problem.m)


# ------------------------------------------------------------------------------- the Python LM loop of the row-sharded solve
LM_FREE = [n for n in NAMES if TC.cases()[n].kind == "lm" and not TC.cases()[n].bounded]


@pytest.mark.parametrize("name", LM_FREE)
def test_rowshard_python_loop(name):
    """rowshard.lm_lsmr on one rank with the numpy backend: counts, flags and the minimizer of the LSMR-certified case."""
    from lsq_amd import rowshard as rs
    z = TC.certify(name, "lsmr")
    c = z.case
    p = c.make()
    S = sp.csc_matrix((np.ones(c.m * c.n), np.tile(np.arange(c.m), c.n), np.arange(c.n + 1) * c.m), shape=(c.m, c.n))

    def g_local(data, x):
        J = np.zeros((c.m, c.n))
        p.g(J, x)
        data[:] = J.reshape(-1, order="F")

    B = rs.NumpyBackend(S, p.f, g_local)
    o = {k: v for k, v in c.opts.items() if k not in ("lower", "upper", "delta")}
    delta = 10.0 if c.opts["delta"] is None else c.opts["delta"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if z.f64.status == R.ENONFINITE:
            with pytest.raises(FloatingPointError):
                rs.lm_lsmr(B, rs.Comm(), c.x0, c.m, delta=delta, **o)
            return
        r = rs.lm_lsmr(B, rs.Comm(), c.x0, c.m, delta=delta, **o)
    got = (r.iterations, bool(r.converged), bool(r.x_converged), bool(r.f_converged), bool(r.g_converged), r.f_calls, r.g_calls)
    assert got == TC.summary(z.f64)[1:], name
    assert r.lsmr_iterations == sum(rec["inner"] for rec in z.f64.its) // 2
    assert np.max(np.abs(r.minimizer - z.f64.x)) <= 1e-9 * max(1.0, np.max(np.abs(z.f64.x)))


def test_comparisons_at_rounding_level():
    """The device tier scales the floor of rho (and of a delta LM computes from it) and of the gradient norm by their condition
    numbers.  Where one exceeds TC.COND_CAP the comparison is of rounding errors and is not coverage: this counts them, so
    that the tier cannot drift into comparing noise.  They are the late iterations of fits that converge (and the steps at
    the MIN_DELTA floor, where x - dx == x)."""
    total = big = at_floor = 0
    worst = {}
    runs = [(n, TC.certify(n, s), max(TC.M, TC.N)) for n in NAMES for s in ("direct", "lsmr")]
    runs += [("spread/%d/%s/%d" % (n, k, b), TC.certify_spread(n, k, b), n + 3) for n, k, b in SPREAD]
    for name, z, kdim in runs:
        if z.f64.status != R.OK:
            continue
        for i, what, hp, cond, bound in TC.trajectory_pieces(z.f64, z.ld, z.oracle.trace, kdim):
            total += 1
            if cond > TC.COND_CAP and name.endswith("_to_floor"):
                at_floor += 1       # the two cases that shrink delta to 1e-16 are there for the delta sequence, which is exact
            elif cond > TC.COND_CAP:
                big += 1
                worst[what] = max(worst.get(what, 0.0), cond)
    print("TRCOND %d of %d comparisons have a condition factor beyond %.0e (and %d in the two *_to_floor cases); largest per "
          "quantity %s" % (big, total, TC.COND_CAP, at_floor, worst))
    assert big <= 0.02 * total, (big, total)
