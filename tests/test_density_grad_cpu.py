"""CPU checks of the float64 restatement of the window sum's gradient (tests/density_grad_ref.py), which the GPU tests of
dmcf_frs_window_sum_backward compare against: its gradient against central finite differences for every window, its forward
against the oracle's compute_density."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import density_grad_ref as R  # noqa: E402

RADIUS = 0.3


def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(0, 1, size=(n, 3)).astype(np.float32)


def _value(oracle_pairs, points, queries, name, G, same):
    idx, rs = oracle_pairs
    ws = R.WindowSum(points, points if same else queries, idx, rs, RADIUS, name, same=same)
    return float((ws.out.detach().numpy() * G).sum())


@pytest.mark.parametrize("same", [False, True], ids=["distinct", "same"])
@pytest.mark.parametrize("name", R.WINDOWS)
def test_gradient_against_finite_differences(oracle, name, same):
    pts = _cloud(150, 1)
    qs = pts if same else _cloud(80, 2)
    if not same:
        qs[:5] = pts[:5]  # coincident pairs: dropped by the sqrt-based windows, a zero term otherwise
    idx, rs, _ = oracle.fixed_radius_search(pts, qs, RADIUS)
    assert 5 < len(idx) / len(qs) < 30
    G = np.random.default_rng(3).normal(size=len(qs))
    ws = R.WindowSum(pts, qs, idx, rs, RADIUS, name, same=same)
    gp, gq, ap, aq = ws.grads(G)
    assert np.isfinite(gp).all() and (gq is None or np.isfinite(gq).all())
    assert (np.abs(gp) <= ap * (1 + 1e-12) + 1e-300).all()
    h = 1e-6
    rng = np.random.default_rng(4)
    P, Q = pts.astype(np.float64), qs.astype(np.float64)
    for which, g in (("points", gp),) + (() if same else (("queries", gq),)):
        base = P if which == "points" else Q
        for _ in range(12):
            i, a = int(rng.integers(base.shape[0])), int(rng.integers(3))
            vals = []
            for sgn in (+1, -1):
                moved = base.copy()
                moved[i, a] += sgn * h
                args = (moved, Q) if which == "points" else (P, moved)
                vals.append(_value((idx, rs), args[0], args[1], name, G, same))
            fd = (vals[0] - vals[1]) / (2 * h)
            scale = max(np.abs(g).max(), 1.0)
            assert abs(fd - g[i, a]) <= 1e-5 * scale, (which, i, a, fd, g[i, a])


@pytest.mark.parametrize("name", ["poly6", "cubic", "linear", "peak", None])
def test_forward_against_oracle(oracle, name):
    pts, qs = _cloud(500, 5), _cloud(200, 6)
    idx, rs, _ = oracle.fixed_radius_search(pts, qs, RADIUS)
    ws = R.WindowSum(pts, qs, idx, rs, RADIUS, "explicit" if name is None else name)
    out = ws.out.detach().numpy()
    if name is None:  # (the reference's identity branch: the sum of q = d^2 / R^2)
        out = out / (np.float32(RADIUS) ** 2)
    ref = oracle.compute_density(qs, pts, RADIUS, name)
    np.testing.assert_allclose(out, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())


def test_coincident_pairs_and_empty_lists():
    pts = _cloud(4, 7)
    idx, rs = np.arange(4), np.arange(5)  # every point paired with itself only
    for name in R.WINDOWS:
        g, _, a, _ = R.WindowSum(pts, pts, idx, rs, RADIUS, name, same=True).grads(np.ones(4))
        assert (g == 0).all() and (a == 0).all(), name
    ws = R.WindowSum(pts, _cloud(3, 8), np.zeros(0, np.int64), np.zeros(4, np.int64), RADIUS, "poly6")
    gp, gq, ap, aq = ws.grads(np.ones(3))
    assert gp.shape == (4, 3) and gq.shape == (3, 3) and not gp.any() and not gq.any() and not ap.any() and not aq.any()
