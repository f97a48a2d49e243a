"""tests/fireref.py -- the NumPy definition of the minimiser -- on a potential with a known answer: an anisotropic
quadratic bowl E = 1/2 sum k_ic (x_ic - x0_ic)^2 with unequal masses (so the mixing step moves the centre of mass, as in
the alloy).  No GPU, no oracle."""
import numpy as np
import pytest

import fireref


def _bowl(n=12, seed=3, kmax=40.0):
    rng = np.random.default_rng(seed)
    k = rng.uniform(1.0, kmax, size=(n, 3))
    x0 = rng.uniform(-2.0, 2.0, size=(n, 3))
    m = rng.uniform(1.0, 8.0, size=n)

    def fe(x):
        d = x - x0
        return -k * d, 0.5 * float((k * d * d).sum())
    return fe, x0, m, rng


def _trace(fe, x, m, dt, **kw):
    rows = []
    run_kw = dict(etol=0.0, ftol=1e-9, maxiter=5000, maxeval=100000)
    run_kw.update({k: kw.pop(k) for k in list(kw) if k in run_kw})
    last = dict(x=np.array(x, dtype=float), v=np.zeros_like(x), dt=dt, f=fe(np.asarray(x, dtype=float))[0])

    def record(s, f):
        rows.append(dict(iter=s.iter, dt=s.dt, dtv=s.dtv, mixed=s.mixed, x=s.x.copy(), v=s.v.copy(), x_before=last["x"],
                         v_before=last["v"], dt_before=last["dt"], f_used=last["f"]))
        last.update(x=s.x.copy(), v=s.v.copy(), dt=s.dt, f=f.copy())
    out = fireref.minimize(fe, x, m, dt, 1.0, record=record, **run_kw, **kw)
    return out, rows


def test_converges_to_the_known_minimum():
    fe, x0, m, rng = _bowl()
    out, rows = _trace(fe, x0 + rng.uniform(-0.5, 0.5, size=x0.shape), m, 0.01)
    assert out["stop"] == fireref.FTOL and out["fnorm"] < 1e-9
    assert np.abs(out["x"] - x0).max() < 1e-9          # |x - x0| <= |f| / k_min, k_min >= 1
    assert out["e_final"] < 1e-18 and out["e_final"] <= out["e_initial"]
    assert out["iterations"] == out["evaluations"] == len(rows)
    assert len(out["negatives"]) >= 2 and out["negatives"][0] == 1     # the start from rest is the first P <= 0


def test_dt_stays_between_dtmin_and_dtmax_and_both_ends_are_reached():
    fe, x0, m, rng = _bowl()
    dt0 = 0.002
    out, rows = _trace(fe, x0 + rng.uniform(-0.5, 0.5, size=x0.shape), m, dt0)     # soft for this dt: dt grows to dtmax
    dts = np.array([r["dt"] for r in rows])
    assert dts.max() <= 10.0 * dt0 and dts.min() >= 0.02 * dt0
    assert dts.max() == 10.0 * dt0
    fe, x0, m, rng = _bowl(kmax=4000.0)
    dt0 = 0.5                                                                   # far too long: dt shrinks to the floor
    out, rows = _trace(fe, x0 + rng.uniform(-0.5, 0.5, size=x0.shape), m, dt0, initialdelay=False, maxiter=400)
    dts = np.array([r["dt"] for r in rows])
    assert dts.max() <= 10.0 * dt0 and dts.min() >= 0.02 * dt0
    assert dts.min() < 2.0 * 0.02 * dt0                                         # the next halving would cross dtmin


def test_velocities_restart_from_rest_after_every_negative_power():
    fe, x0, m, rng = _bowl()
    out, rows = _trace(fe, x0 + rng.uniform(-0.5, 0.5, size=x0.shape), m, 0.01)
    neg = [r for r in rows if not r["mixed"]]
    assert len(neg) >= 2
    for r in neg:      # v = 0, then the kick alone; x went half the previous step back first
        kick = r["dtv"] * 1.0 * r["f_used"] / m[:, None]
        assert np.array_equal(r["v"], kick)
    for a, b in zip(rows, rows[1:]):
        if not b["mixed"]:
            back = b["x_before"] - 0.5 * a["dtv"] * b["v_before"]
            assert np.abs(b["x"] - (back + b["dtv"] * b["v"])).max() < 1e-14


def test_dmax_limits_the_step_of_the_velocities_an_iteration_starts_from():
    """The limit is taken from the velocities before the kick (module docstring), so that is what is asserted exactly;
    the move itself exceeds dmax only by what the kick and the mixing of the same iteration add."""
    fe, x0, m, rng = _bowl()
    dmax = 0.02
    out, rows = _trace(fe, x0 + rng.uniform(-3.0, 3.0, size=x0.shape), m, 0.05, dmax=dmax)
    assert out["stop"] == fireref.FTOL
    limited = 0
    for r in rows:
        vmax = 0.0 if not r["mixed"] else np.abs(r["v_before"]).max()
        assert r["dtv"] * vmax <= dmax * (1.0 + 1e-15)
        assert r["dtv"] <= r["dt"]
        limited += r["dtv"] < r["dt"]
        move = r["dtv"] * np.abs(r["v"]).max()                      # x += dtv v
        added = r["dtv"] * np.abs(r["v"] - (r["v_before"] if r["mixed"] else 0.0)).max()
        assert move <= dmax + added + 1e-15
    assert limited >= 5


def test_no_dt_shrink_inside_the_initial_delay():
    fe, x0, m, rng = _bowl(kmax=4000.0)
    x = x0 + rng.uniform(-0.5, 0.5, size=x0.shape)
    out, rows = _trace(fe, x, m, 0.05, maxiter=60)
    early = [r for r in rows if r["iter"] < 20]
    assert any(not r["mixed"] for r in early if r["iter"] > 1)          # overshoots inside the delay ...
    assert all(r["dt"] == 0.05 for r in early)                          # ... leave dt alone
    assert any(r["dt"] < r["dt_before"] for r in rows if r["iter"] >= 20)
    out, rows = _trace(fe, x, m, 0.05, maxiter=60, initialdelay=False)
    assert any(r["dt"] < r["dt_before"] for r in rows if r["iter"] < 20)


@pytest.mark.parametrize("want", [fireref.FTOL, fireref.ETOL, fireref.MAXITER, fireref.MAXEVAL])
def test_each_stop_criterion_is_reachable(want):
    fe, x0, m, rng = _bowl()
    x = x0 + rng.uniform(-0.5, 0.5, size=x0.shape)
    kw = {fireref.FTOL: dict(etol=0.0, ftol=1e-6, maxiter=5000, maxeval=100000),
          fireref.ETOL: dict(etol=1e-10, ftol=0.0, maxiter=5000, maxeval=100000),
          fireref.MAXITER: dict(etol=0.0, ftol=0.0, maxiter=37, maxeval=100000),
          fireref.MAXEVAL: dict(etol=0.0, ftol=0.0, maxiter=5000, maxeval=37)}[want]
    out = fireref.minimize(fe, x, m, 0.01, 1.0, **kw)
    assert out["stop"] == want
    if want in (fireref.MAXITER, fireref.MAXEVAL):
        assert out["iterations"] == out["evaluations"] == 37
    if want == fireref.ETOL:
        assert out["iterations"] - out["state"].last_negative > 20
        assert abs(out["e_final"] - out["e_previous"]) < 1e-10 * 0.5 * (abs(out["e_final"]) + abs(out["e_previous"]) + 1e-8)
    if want == fireref.FTOL:
        assert out["fnorm"] < 1e-6
    assert fireref.minimize(fe, x, m, 0.01, 1.0, 0.0, 0.0, 0, 10)["iterations"] == 0
