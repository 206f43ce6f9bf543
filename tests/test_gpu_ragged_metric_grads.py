"""Gradients of the ragged point-set losses on the GPU (ABI 2.25): the recording ragged EMD (dmcf_emd_ragged_with_levels /
dmcf_emd_ragged_backward) and the recording ragged nn_distance (dmcf_nn_distance_backward over the concatenated rows) against
the un-batched recording calls on every item alone, BIT FOR BIT, and against the float64 restatement of
tests/metric_grads_ref.py within the bar of tests/test_gpu_metric_grads.py; the loss functions with row splits, and the
pipeline key train_set_losses.

Shapes: the item list of tests/test_gpu_emd_ragged.py -- one lane; a partial and a full 256-row block and one row over; items
empty on one side and on both; the workload's 2,025-point scene; and (20000, 7000), whose plan has two-tile chunks on both
sides (tests/test_ragged_metric_grads_abi.py asserts the plans).  nn_distance refuses an item with exactly one empty set, so its
batch leaves (0, 5) and (5, 0) out."""
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import metric_grads_ref as G  # noqa: E402
from test_gpu_emd_ragged import SIZES, _Counting, _splits  # noqa: E402
from test_gpu_metric_grads import WORST, _close  # noqa: E402  (the bar 16 2^-24 A, taken from there)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NN_SIZES = [s for s in SIZES if (s[0] == 0) == (s[1] == 0)]


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _batch(sizes, seed, dim=3):
    rng = np.random.default_rng(seed)
    a = [rng.uniform(0, 1, size=(n, dim)).astype(np.float32) for n, _ in sizes]
    b = [(rng.uniform(0, 1, size=(m, dim)) * 0.8 + 0.1).astype(np.float32) for _, m in sizes]
    return a, b, _splits([n for n, _ in sizes]), _splits([m for _, m in sizes])


def _cat(parts, dim=3):
    return np.concatenate(parts) if parts else np.zeros((0, dim), np.float32)


def _emd_ragged_grads(a, b, rs1, rs2, w, need1=True, need2=True):
    from dmcf_amd import ops
    A, B = _t(_cat(a), need1), _t(_cat(b), need2)
    cost = ops.emd_ragged_recording(A, B, rs1, rs2)
    assert cost.grad_fn is not None
    (cost * w).sum().backward()
    return cost.detach(), A.grad, B.grad


def _emd_item_grads(x1, x2, wk):
    """The un-batched recording call on one item alone (the parent's code path) -> its two gradients."""
    from dmcf_amd import ops
    p, q = _t(x1[None], True), _t(x2[None], True)
    (ops.emd(p, q)[0] * wk).backward()
    return p.grad[0], q.grad[0]


@pytest.fixture(scope="module")
def emd():
    """The batch, the recording ragged call's cost and gradients under random weights, and the un-batched recording call on
    every item with both sets non-empty, computed once."""
    from dmcf_amd import ops
    a, b, rs1, rs2 = _batch(SIZES, 25)
    w = _t(np.random.default_rng(26).normal(size=len(SIZES)))
    cost, g1, g2 = _emd_ragged_grads(a, b, rs1, rs2, w)
    plain = ops.emd_ragged(_t(_cat(a)), _t(_cat(b)), rs1, rs2)
    items = [_emd_item_grads(a[k], b[k], w[k]) if n and m else None for k, (n, m) in enumerate(SIZES)]
    yield dict(a=a, b=b, rs1=rs1, rs2=rs2, w=w, cost=cost, g1=g1, g2=g2, plain=plain, items=items)
    print("\nworst err/bar:", {k: float("%.3g" % v) for k, v in sorted(WORST.items()) if k.startswith("ragged")})


# ---- 1. the EMD bit contract ---------------------------------------------------------------------------------------------------
def test_emd_gradients_have_the_per_item_calls_bits(emd):
    rs1, rs2, g1, g2 = emd["rs1"], emd["rs2"], emd["g1"], emd["g2"]
    assert g1.shape == (rs1[-1], 3) and g2.shape == (rs2[-1], 3) and g1.dtype == torch.float32
    assert torch.equal(emd["cost"], emd["plain"])
    for k, (n, m) in enumerate(SIZES):
        u, v = g1[rs1[k]:rs1[k + 1]], g2[rs2[k]:rs2[k + 1]]
        if emd["items"][k] is None:  # an empty partner set: exact zeros
            assert not u.any() and not v.any(), (k, SIZES[k])
            continue
        want1, want2 = emd["items"][k]
        assert torch.equal(u, want1), (k, SIZES[k], float((u - want1).abs().max()))
        assert torch.equal(v, want2), (k, SIZES[k], float((v - want2).abs().max()))
        assert u.any() and v.any(), (k, SIZES[k])


# ---- 2. the Chamfer bit contract -----------------------------------------------------------------------------------------------
def _nn_ragged_grads(a, b, rs1, rs2, g1, g2, dim=3):
    from dmcf_amd import ops
    A, B = _t(_cat(a, dim), True), _t(_cat(b, dim), True)
    d1, i1, d2, i2 = ops.nn_distance_ragged(A, B, rs1, rs2, record=True)
    assert d1.grad_fn is not None and d2.grad_fn is not None and not i1.requires_grad and not i2.requires_grad
    loss = (0 if g1 is None else (d1 * g1).sum()) + (0 if g2 is None else (d2 * g2).sum())
    loss.backward()
    return (d1.detach(), i1, d2.detach(), i2), A.grad, B.grad


def _nn_item_grads(x1, x2, g1, g2):
    from dmcf_amd import ops
    p, q = _t(x1[None], True), _t(x2[None], True)
    d1, _, d2, _ = ops.nn_distance(p, q)
    loss = (0 if g1 is None else (d1[0] * g1).sum()) + (0 if g2 is None else (d2[0] * g2).sum())
    loss.backward()
    return p.grad[0], q.grad[0]


@pytest.fixture(scope="module")
def nn():
    a, b, rs1, rs2 = _batch(NN_SIZES, 27)
    rng = np.random.default_rng(28)
    return dict(a=a, b=b, rs1=rs1, rs2=rs2, g1=_t(rng.normal(size=rs1[-1])), g2=_t(rng.normal(size=rs2[-1])))


@pytest.mark.parametrize("case", ["both", "only1", "only2"])
def test_nn_distance_gradients_have_the_per_item_calls_bits(nn, case):
    from dmcf_amd import ops
    a, b, rs1, rs2 = nn["a"], nn["b"], nn["rs1"], nn["rs2"]
    g1 = None if case == "only2" else nn["g1"]
    g2 = None if case == "only1" else nn["g2"]
    out, u, v = _nn_ragged_grads(a, b, rs1, rs2, g1, g2)
    plain = ops.nn_distance_ragged(_t(_cat(a)), _t(_cat(b)), rs1, rs2)
    for x, y in zip(out, plain):
        assert torch.equal(x, y)
    for k, (n, m) in enumerate(NN_SIZES):
        if n == 0:
            continue
        want1, want2 = _nn_item_grads(a[k], b[k], None if g1 is None else g1[rs1[k]:rs1[k + 1]],
                                      None if g2 is None else g2[rs2[k]:rs2[k + 1]])
        assert torch.equal(u[rs1[k]:rs1[k + 1]], want1), (case, k, NN_SIZES[k])
        assert torch.equal(v[rs2[k]:rs2[k + 1]], want2), (case, k, NN_SIZES[k])
    assert u.any() and v.any()


def test_nn_distance_collapsed_clouds_as_items_1_and_2():
    """The clouds of test_nn_distance_backward_collapsed_cloud as items 1 and 2 behind a small item: one target gathers more
    than 256 sources (the workgroup path of the inversion), at sorted positions the un-batched call never sees."""
    rng = np.random.default_rng(95)
    n, m = 3000, 5000
    x1 = rng.uniform(size=(2, n, 3))
    x2 = rng.uniform(size=(2, m, 3)) * 0.1 + 10.0
    x2[1, :100] = x1[1, :100] + 1e-3
    a = [rng.uniform(size=(37, 3)).astype(np.float32), np.float32(x1[0]), np.float32(x1[1])]
    b = [rng.uniform(size=(41, 3)).astype(np.float32), np.float32(x2[0]), np.float32(x2[1])]
    rs1, rs2 = _splits([len(x) for x in a]), _splits([len(x) for x in b])
    g1, g2 = _t(rng.normal(size=rs1[-1])), _t(rng.normal(size=rs2[-1]))
    (_, i1, _, i2), u, v = _nn_ragged_grads(a, b, rs1, rs2, g1, g2)
    assert np.bincount(_np(i2)[rs2[1]:rs2[2]]).max() > 256 and np.bincount(_np(i1)[rs1[1]:rs1[2]]).max() > 256
    for k in range(3):
        want1, want2 = _nn_item_grads(a[k], b[k], g1[rs1[k]:rs1[k + 1]], g2[rs2[k]:rs2[k + 1]])
        assert torch.equal(u[rs1[k]:rs1[k + 1]], want1), k
        assert torch.equal(v[rs2[k]:rs2[k + 1]], want2), k


# ---- 3. against float64 --------------------------------------------------------------------------------------------------------
def test_emd_gradients_against_float64(emd):
    """match_cost_grad of tests/metric_grads_ref.py on the item's ops.approx_match match, every item up to (2025, 2025)."""
    from dmcf_amd import ops
    rs1, rs2 = emd["rs1"], emd["rs2"]
    for k, (n, m) in enumerate(SIZES[:-1]):
        if n == 0 or m == 0:
            continue
        x1, x2 = emd["a"][k][None], emd["b"][k][None]
        match = ops.approx_match(_t(x1), _t(x2))
        r1, r2, A1, A2 = G.match_cost_grad(x1, x2, _np(match).astype(np.float64), _np(emd["w"][k:k + 1]))
        _close(emd["g1"][rs1[k]:rs1[k + 1]], r1[0], A1[0], "ragged_emd")
        _close(emd["g2"][rs2[k]:rs2[k + 1]], r2[0], A2[0], "ragged_emd")
    print("worst err / bar, ragged emd:", WORST["ragged_emd"])


def test_nn_distance_gradients_against_float64(nn):
    a, b, rs1, rs2 = nn["a"], nn["b"], nn["rs1"], nn["rs2"]
    (_, i1, _, i2), u, v = _nn_ragged_grads(a, b, rs1, rs2, nn["g1"], nn["g2"])
    for k, (n, m) in enumerate(NN_SIZES[:-1]):
        if n == 0:
            continue
        s1, s2 = slice(rs1[k], rs1[k + 1]), slice(rs2[k], rs2[k + 1])
        f64 = lambda x: np.asarray(x, dtype=np.float64)[None]  # noqa: E731
        r1, r2, A1, A2 = G.nn_distance_grad(f64(a[k]), f64(b[k]), f64(_np(nn["g1"][s1])), f64(_np(nn["g2"][s2])),
                                            _np(i1[s1])[None] - rs2[k], _np(i2[s2])[None] - rs1[k])
        _close(u[s1], r1[0], A1[0], "ragged_nn")
        _close(v[s2], r2[0], A2[0], "ragged_nn")
    print("worst err / bar, ragged nn_distance:", WORST["ragged_nn"])


# ---- 4. one side only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 2])
def test_one_side_only(emd, side):
    _, g1, g2 = _emd_ragged_grads(emd["a"], emd["b"], emd["rs1"], emd["rs2"], emd["w"], need1=side == 1, need2=side == 2)
    if side == 1:
        assert g2 is None and torch.equal(g1, emd["g1"])
    else:
        assert g1 is None and torch.equal(g2, emd["g2"])


def test_a_batch_without_a_pair_and_the_backward_helpers_operands():
    """Items that are empty on one side only: zero costs, zero levels and zero gradients (the library zeroes them, no kernel
    runs).  And ops.emd_ragged_backward checks the shapes, dtypes and devices of its operands before anything is launched."""
    from dmcf_amd import _lib, ops
    A, B = _t(np.ones((5, 3)), True), _t(np.ones((5, 3)), True)
    rs1, rs2 = [0, 5, 5], [0, 0, 5]
    cost = ops.emd_ragged_recording(A, B, rs1, rs2)
    assert cost.grad_fn is not None and not cost.any()
    (cost * _t(np.float32([2.0, float("inf")]))).sum().backward()
    assert A.grad.shape == (5, 3) and not A.grad.any() and not B.grad.any()
    _, levels = ops.emd_ragged_with_levels(A.detach(), B.detach(), rs1, rs2)
    assert levels.shape == (ops.EMD_LEVELS, 10) and not levels.any()
    x1, x2 = torch.zeros(5, 3, device=DEV), torch.zeros(4, 3, device=DEV)
    lv, gc = torch.zeros(10, 9, device=DEV), torch.ones(2, device=DEV)
    with pytest.raises(ValueError):
        ops.emd_ragged_backward(x1, x2, [0, 2, 5], [0, 1, 4], lv[:, :8], gc)
    with pytest.raises(ValueError):
        ops.emd_ragged_backward(x1, x2, [0, 2, 5], [0, 1, 4], lv, gc[:1])
    with pytest.raises(TypeError):
        ops.emd_ragged_backward(x1, x2, [0, 2, 5], [0, 1, 4], lv.double(), gc)
    with pytest.raises(_lib.DmcfError):
        ops.emd_ragged_backward(x1, x2, [0, 2, 5], [0, 1, 4], lv, gc.cpu())
    with pytest.raises(ValueError):
        ops.emd_ragged_with_levels(x1[None], x2[None], [0, 5], [0, 4])  # a padded batch: not the ragged layout
    g1, g2 = ops.emd_ragged_backward(x1, x2, [0, 2, 5], [0, 1, 4], lv, gc, need2=False)
    assert g1.shape == (5, 3) and g2 is None


# ---- 5. the recording forward runs only when a gradient is wanted -------------------------------------------------------------
def test_recording_forward_only_when_wanted(emd, monkeypatch):
    from dmcf_amd import _lib, ops
    a, b, rs1, rs2 = _cat(emd["a"]), _cat(emd["b"]), emd["rs1"], emd["rs2"]
    counting = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    calls = lambda name: counting.calls.get(name, 0)  # noqa: E731
    with torch.no_grad():
        plain = ops.emd_ragged_recording(_t(a, True), _t(b, True), rs1, rs2)
    assert calls("dmcf_emd_ragged_with_levels") == 0 and calls("dmcf_emd_ragged") == 1
    plain2 = ops.emd_ragged_recording(_t(a), _t(b), rs1, rs2)  # grad mode on, nothing requires grad
    assert calls("dmcf_emd_ragged_with_levels") == 0 and calls("dmcf_emd_ragged") == 2
    rec = ops.emd_ragged_recording(_t(a), _t(b, True), rs1, rs2)
    assert calls("dmcf_emd_ragged_with_levels") == 1 and calls("dmcf_emd_ragged") == 2
    assert rec.grad_fn is not None and plain.grad_fn is None and plain2.grad_fn is None
    assert torch.equal(rec.detach(), plain) and torch.equal(plain, plain2) and torch.equal(plain, emd["plain"])
    rec.sum().backward()
    assert calls("dmcf_emd_ragged_backward") == 1 and calls("dmcf_emd_backward") == 0
    # the recorded ratios: [10, n_total + m_total], zeros in the rows of an item with an empty set
    cost, levels = ops.emd_ragged_with_levels(_t(a), _t(b), rs1, rs2)
    assert torch.equal(cost, plain) and levels.shape == (ops.EMD_LEVELS, rs1[-1] + rs2[-1])
    lv = _np(levels)
    for k, (n, m) in enumerate(SIZES):
        rows = np.r_[rs1[k]:rs1[k + 1], rs1[-1] + rs2[k]:rs1[-1] + rs2[k + 1]]
        if n == 0 or m == 0:
            assert (lv[:, rows] == 0).all(), k
        else:
            assert (lv[:, rows] > 0).any() and np.isfinite(lv[:, rows]).all(), k
    # ... and they are what the un-batched recording forward records for an item alone
    k = 6
    _, one = ops.emd_with_levels(_t(emd["a"][k][None]), _t(emd["b"][k][None]))
    n = SIZES[k][0]
    assert torch.equal(levels[:, rs1[k]:rs1[k + 1]], one[0][:, :n])
    assert torch.equal(levels[:, rs1[-1] + rs2[k]:rs1[-1] + rs2[k + 1]], one[0][:, n:])


# ---- 6. determinism and permutation --------------------------------------------------------------------------------------------
def test_repeatable_and_permuting_the_items_permutes_the_rows(emd, nn):
    _, g1, g2 = _emd_ragged_grads(emd["a"], emd["b"], emd["rs1"], emd["rs2"], emd["w"])
    assert torch.equal(g1, emd["g1"]) and torch.equal(g2, emd["g2"])
    order = [10, 3, 8, 0, 9, 5, 1, 7, 6, 2, 4]
    assert sorted(order) == list(range(len(SIZES)))
    a, b = [emd["a"][k] for k in order], [emd["b"][k] for k in order]
    p1, p2 = _splits([len(x) for x in a]), _splits([len(x) for x in b])
    _, h1, h2 = _emd_ragged_grads(a, b, p1, p2, emd["w"][torch.tensor(order, device=DEV)])
    for j, k in enumerate(order):
        assert torch.equal(h1[p1[j]:p1[j + 1]], emd["g1"][emd["rs1"][k]:emd["rs1"][k + 1]]), (j, k)
        assert torch.equal(h2[p2[j]:p2[j + 1]], emd["g2"][emd["rs2"][k]:emd["rs2"][k + 1]]), (j, k)
    # nn_distance: two identical calls, and the items in reverse
    _, u, v = _nn_ragged_grads(nn["a"], nn["b"], nn["rs1"], nn["rs2"], nn["g1"], nn["g2"])
    _, u2, v2 = _nn_ragged_grads(nn["a"], nn["b"], nn["rs1"], nn["rs2"], nn["g1"], nn["g2"])
    assert torch.equal(u, u2) and torch.equal(v, v2)
    rev = list(range(len(NN_SIZES)))[::-1]
    a, b = [nn["a"][k] for k in rev], [nn["b"][k] for k in rev]
    q1, q2 = _splits([len(x) for x in a]), _splits([len(x) for x in b])
    r1, r2 = nn["rs1"], nn["rs2"]
    _, x, y = _nn_ragged_grads(a, b, q1, q2, torch.cat([nn["g1"][r1[k]:r1[k + 1]] for k in rev]),
                               torch.cat([nn["g2"][r2[k]:r2[k + 1]] for k in rev]))
    for j, k in enumerate(rev):
        assert torch.equal(x[q1[j]:q1[j + 1]], u[r1[k]:r1[k + 1]]) and torch.equal(y[q2[j]:q2[j + 1]], v[r2[k]:r2[k + 1]]), (j, k)


# ---- 7. the loss functions -----------------------------------------------------------------------------------------------------
def test_losses_with_splits_equal_the_per_item_losses(emd, nn):
    from dmcf_amd.utils.tools.losses import emd_loss, emd_loss_ragged
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    # EMD: y_true = the first sets, y_pred = the second
    T, P = _t(_cat(emd["a"]), True), _t(_cat(emd["b"]), True)
    rs1, rs2 = emd["rs1"], emd["rs2"]
    got = emd_loss_ragged(T, P, rs1, rs2, record=True)
    assert got.shape == (len(SIZES),) and got.grad_fn is not None
    assert torch.equal(got.detach(), emd_loss(T.detach(), P.detach(), true_row_splits=rs1, pred_row_splits=rs2))
    got.sum().backward()
    for k, (n, m) in enumerate(SIZES):
        if n == 0 or m == 0:
            assert float(got[k].detach()) == 0.0 and not T.grad[rs1[k]:rs1[k + 1]].any() and not P.grad[rs2[k]:rs2[k + 1]].any()
            continue
        t, p = _t(emd["a"][k][None], True), _t(emd["b"][k][None], True)
        want = emd_loss(t, p)
        want.sum().backward()
        assert torch.equal(got[k].detach(), want[0].detach()), (k, float(got[k]), float(want[0]))
        assert torch.equal(T.grad[rs1[k]:rs1[k + 1]], t.grad[0]) and torch.equal(P.grad[rs2[k]:rs2[k + 1]], p.grad[0]), k
    # Chamfer
    T, P = _t(_cat(nn["a"]), True), _t(_cat(nn["b"]), True)
    rs1, rs2 = nn["rs1"], nn["rs2"]
    got = chamfer_loss(T, P, true_row_splits=rs1, pred_row_splits=rs2, record=True)
    assert got.shape == (len(NN_SIZES),) and got.grad_fn is not None
    assert torch.equal(got.detach(), chamfer_loss(T.detach(), P.detach(), true_row_splits=rs1, pred_row_splits=rs2))
    got.sum().backward()
    for k, (n, m) in enumerate(NN_SIZES):
        if n == 0:
            assert float(got[k].detach()) == 0.0
            continue
        t, p = _t(nn["a"][k][None], True), _t(nn["b"][k][None], True)
        want = chamfer_loss(t, p)
        want.sum().backward()
        assert torch.equal(got[k].detach(), want[0].detach()), (k, float(got[k]), float(want[0]))
        assert torch.equal(T.grad[rs1[k]:rs1[k + 1]], t.grad[0]) and torch.equal(P.grad[rs2[k]:rs2[k + 1]], p.grad[0]), k
    with pytest.raises(ValueError):  # exactly one empty set: nn_distance's refusal
        chamfer_loss(T.detach()[:5], P.detach()[:3], true_row_splits=[0, 5, 5], pred_row_splits=[0, 2, 3], record=True)


@pytest.mark.parametrize("which", ["chamfer", "emd"])
def test_ten_gradient_steps_follow_the_items_stepped_alone(which):
    """Three items of different sizes: the ragged batch's trajectory is, bit for bit, that of every item stepped alone (the
    learning rates of test_gradient_steps_reduce_distance)."""
    from dmcf_amd.utils.tools.losses import emd_loss, emd_loss_ragged
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    rng = np.random.default_rng(80)
    sizes = [(400, 400), (300, 513), (650, 401)]  # (target points, moving points)
    tgt = [_t(rng.uniform(size=(n, 3))) for n, _ in sizes]
    start = [np.float32(rng.uniform(size=(m, 3)) * 0.5 + 0.5) for _, m in sizes]
    trs, prs = _splits([n for n, _ in sizes]), _splits([m for _, m in sizes])
    lr = 100.0 if which == "chamfer" else 12.0
    if which == "chamfer":
        ragged = lambda T, X: chamfer_loss(T, X, true_row_splits=trs, pred_row_splits=prs, record=True)  # noqa: E731
        alone = chamfer_loss
    else:
        ragged = lambda T, X: emd_loss_ragged(T, X, trs, prs, record=True)  # noqa: E731
        alone = emd_loss
    T, X = torch.cat(tgt), _t(np.concatenate(start), True)
    xs = [_t(s[None], True) for s in start]
    first = float(ragged(T, X)[0].detach())
    for step in range(10):
        X.grad = None
        ragged(T, X).sum().backward()
        with torch.no_grad():
            X -= lr * X.grad
        for k, x in enumerate(xs):
            x.grad = None
            alone(tgt[k][None], x).sum().backward()
            with torch.no_grad():
                x -= lr * x.grad
            assert torch.equal(X.detach()[prs[k]:prs[k + 1]], x.detach()[0]), (which, step, k)
    last = ragged(T, X).detach()
    assert torch.isfinite(last).all() and float(last[0]) < 0.9 * first  # (item 0 has that test's sizes)


# ---- 8. 2-D sets ---------------------------------------------------------------------------------------------------------------
def test_2d_sets():
    from dmcf_amd import ops
    sizes = [(7, 3), (256, 257), (0, 0), (300, 700)]
    a, b, rs1, rs2 = _batch(sizes, 31, dim=2)
    w = _t(np.float32([0.5, -1.5, 2.0, 1.25]))
    A, B = _t(_cat(a, 2), True), _t(_cat(b, 2), True)
    (ops.emd_ragged_recording(A, B, rs1, rs2) * w).sum().backward()
    assert A.grad.shape == (rs1[-1], 2) and B.grad.shape == (rs2[-1], 2)
    rng = np.random.default_rng(32)
    g1, g2 = _t(rng.normal(size=rs1[-1])), _t(rng.normal(size=rs2[-1]))
    _, u, v = _nn_ragged_grads(a, b, rs1, rs2, g1, g2, dim=2)
    assert u.shape == (rs1[-1], 2) and v.shape == (rs2[-1], 2)
    for k, (n, m) in enumerate(sizes):
        if n == 0:
            continue
        s1, s2 = slice(rs1[k], rs1[k + 1]), slice(rs2[k], rs2[k + 1])
        want1, want2 = _emd_item_grads(a[k], b[k], w[k])
        assert want1.shape == (n, 2) and torch.equal(A.grad[s1], want1) and torch.equal(B.grad[s2], want2), k
        want1, want2 = _nn_item_grads(a[k], b[k], g1[s1], g2[s2])
        assert torch.equal(u[s1], want1) and torch.equal(v[s2], want2), k


# ---- 9. the pipeline key -------------------------------------------------------------------------------------------------------
def test_train_set_losses_in_the_batched_window(monkeypatch):
    from test_gpu_step_batched import _items, _model
    from dmcf_amd import _lib
    from dmcf_amd.pipelines.simulator import Simulator
    from dmcf_amd.utils.tools.losses import emd_loss
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    model = _model("waterramps", loss=True)
    items = _items("waterramps")
    data = dict(pos=[], vel=[], grav=[], box=[], box_normals=[], pre=[0, 0, 0])
    for it in items:
        p0, v0 = it[0].cpu().numpy(), it[1].cpu().numpy()
        data["pos"].append([p0 + k * 0.0025 * v0 + 1e-3 * k for k in range(3)])
        data["vel"].append([v0])
        data["grav"].append([None])
        data["box"].append([it[4].cpu().numpy()])
        data["box_normals"].append([it[5].cpu().numpy()])
    in_pos, in_vel = [it[0] for it in items], [it[1] for it in items]
    time_w = [1.0, 0.5]
    try:
        # without train_batched the key raises before any library call
        def used():
            raise AssertionError("the library was asked for")
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "lib", used)
            with pytest.raises(NotImplementedError, match="train_batched"):
                Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp(), train_set_losses={"chamfer": 1.0})
        res = {}
        for key in (None, {"chamfer": 1.0, "emd": 1.0}):
            sim = Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp(), train_batched=True, train_set_losses=key)
            seen = []
            if key:
                inner = sim._set_loss_columns
                sim._set_loss_columns = lambda pos2, rs, targets: seen.append((pos2, list(rs), targets)) or inner(pos2, rs, targets)
            model.zero_grad()
            loss = sim.window_loss(data, time_w, in_pos, in_vel, [0, 0, 0])
            loss.sum().backward()
            res[bool(key)] = dict(loss=loss.detach(), keys=sim.loss_keys(), seen=seen,
                                  grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    finally:
        model.requires_grad_(False)
    off, on = res[False], res[True]
    k = len(off["keys"])
    assert off["keys"] == list(model.loss_keys()) and on["keys"] == off["keys"] + ["chamfer", "emd"]
    assert off["loss"].shape == (k,) and on["loss"].shape == (k + 2,)
    assert torch.equal(on["loss"][:k], off["loss"])  # the model-loss columns: bit-identical
    # the extra columns, recomputed per sample with the un-batched losses on the recorded pos2 slices, in the same row order
    assert len(on["seen"]) == len(time_w)
    tw = torch.as_tensor(np.asarray(time_w, dtype=np.float32), device=DEV)
    rows = []
    for t, (pos2, rs, targets) in enumerate(on["seen"]):
        for bi, tgt in enumerate(targets):
            p = pos2.detach()[rs[bi]:rs[bi + 1]]
            rows.append(torch.stack([1.0 * chamfer_loss(tgt[None], p[None])[0], 1.0 * emd_loss(tgt[None], p[None])[0]]) * tw[t])
    rows = torch.stack(rows)
    want = rows.sum(0) / (tw.sum() * len(items))
    bound = (rows.shape[0] - 1) * 2.0 ** -24 * rows.abs().sum(0) / (tw.sum() * len(items))
    err = (on["loss"][k:] - want).abs()
    print("extra columns", on["loss"][k:].tolist(), "per sample", want.tolist(), "err", err.tolist(), "bound", bound.tolist())
    assert (want > 0).all() and (err <= bound).all()
    # every weight's gradient is finite, and the terms reach the weights
    assert set(on["grads"]) == set(off["grads"]) and on["grads"]
    assert all(torch.isfinite(g).all() for g in on["grads"].values())
    assert any(not torch.equal(on["grads"][n], off["grads"][n]) for n in on["grads"])
