"""CPU checks of the reference and the bar of tests/test_gpu_cconv_scatter_backward.py (tests/cconv_scatter_backward_ref.py):

* the input-stationary order of evaluation -- T_j first, then dF = W . T_j and dW = sum_j f_j (x) T_j -- is the operator whose
  gradients cconv_backward_ref.grads forms on the forward list: in float64 equal to 1e-12 relative to the value on every
  element whose sum does not cancel (over 90 % of them), to 1e-14 of the sum of the absolute terms on the rest;
* the same restatement in float32 stays inside the bar, and seeded faults of the kind a kernel can have leave it: the last pair of
  a transposed row dropped, two corners swapped, the window of the pair at 0.9995 R set to that at R / 2;
* on every element of every case of the GPU file the derived fixed-point term is at most 1 / 16 of the float part of the bar,
  floor included -- a condition on the cases (change a case's inputs if it breaks, never the cap), so that no GPU test can hide
  behind that term.  Worst shares with these cases: 0.0059 of a feature gradient (7-c31o4m4r2-cut), 0.0005 of a filter gradient."""
import numpy as np
import pytest

import oracle
import cconv_scatter_backward_ref as br
import cconv_scatter_ref as sr

MATRIX = sr.matrix()
# a 24 -> 4 CSR case, a 24 -> 8 padded case and the cut list with the largest fixed-point share; all three with the poly6 window
PICK = [MATRIX[15], MATRIX[24], MATRIX[7]]


@pytest.fixture(scope="module", params=PICK, ids=[m[0] for m in PICK])
def case(request):
    c = sr.Case(**request.param[1])
    assert c.window == "poly6"
    return c, br.Bar(c)


def test_input_stationary_order_is_the_same_operator(case):
    c, b = case
    dW, dF, T = br.restate(c, b.pw, b.G)
    for got, want, A in ((dW, b.want_w, b.A_w), (dF, b.want_f, b.A_f)):
        err = np.abs(got - want)
        # 1e-12 RELATIVE TO THE VALUE wherever the sum does not cancel (|value| >= A / 1000, A the sum of the absolute terms: two
        # float64 orders of one sum differ by some 1e-15 A, i.e. by 1e-12 of such a value at most) ...
        sound = np.abs(want) >= 1e-3 * A
        assert sound.mean() > 0.9
        assert np.all(err[sound] <= 1e-12 * np.abs(want)[sound])
        # ... and where it cancels, where no order of evaluation has digits relative to the value, 1e-14 of A; a sum without
        # terms is an exact zero on both sides
        assert np.all(err[~sound] <= 1e-14 * A[~sound])
        assert np.array_equal(got[A == 0], want[A == 0]) and not got[A == 0].any()
    # rows of input points without pairs (cut rows included) hold no term at all
    lonely = np.bincount(b.pw.j, minlength=c.inp_pos.shape[0]) == 0
    assert lonely.sum() >= 1 + (c.cut_rows.sum() if c.cut else 0)
    assert not T[lonely].any() and not dF[lonely].any() and not b.want_f[lonely].any()


def test_float32_restatement_is_inside_the_bar(case):
    c, b = case
    dW, dF, _ = br.restate(c, b.pw, b.G, np.float32)
    b.check("restated-float32", dW, dF)


def test_dropping_the_last_pair_of_a_row_leaves_the_bar(case):
    """The pair that opens the second 64-pair batch of the 65-pair row: gone, as after an off-by-one in the batch loop (where the
    ball holds fewer than 65 cells: the last pair of the longest row)."""
    c, b = case
    n_j = np.bincount(b.pw.j, minlength=c.inp_pos.shape[0])
    j = c.scene.probes.get(65, int(np.argmax(n_j)))
    mine = np.flatnonzero(b.pw.j == j)
    assert mine.size == (65 if 65 in c.scene.probes else n_j.max()) and mine.size >= 2
    last = mine[np.argmax(b.pw.i[mine])]  # (the transposed row is ordered by output index)
    assert b.pw.a[last] * np.abs(b.G[b.pw.i[last]]).max() > 1e-3
    keep = np.ones(b.pw.i.shape[0], bool)
    keep[last] = False
    dW, dF, _ = br.restate(c, b.pw, b.G, keep=keep)
    assert not b.within(dW, dF)
    assert not b.within(None, dF), "the feature gradient alone must show it"


def test_swapped_corners_leave_the_bar(case):
    c, b = case
    cells = b.pw.cells.copy()
    cells[:, [0, 1]] = cells[:, [1, 0]]  # the x and x + 1 corners trade their weights
    dW, dF, _ = br.restate(c, b.pw, b.G, cells=cells)
    assert not b.within(dW, None) and not b.within(None, dF)


def test_window_of_the_edge_pair_leaves_the_bar(case):
    """The pair at 0.9995 R (window about 1e-9) weighted as if it lay at R / 2."""
    c, b = case
    j, cell = c.scene.edge
    i = int(np.flatnonzero(np.all(c.scene.cells == cell, axis=1))[0])
    p = np.flatnonzero((b.pw.j == j) & (b.pw.i == i))
    assert p.size == 1 and 0.0 <= b.pw.a[p[0]] < 1e-6 * abs(c.window_fac)
    a = b.pw.a.copy()
    a[p[0]] = float(oracle.window("poly6", np.float32([0.25]), c.window_fac)[0])
    dW, dF, _ = br.restate(c, b.pw, b.G, a=a)
    assert not b.within(None, dF)


@pytest.mark.parametrize("cid,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_fixed_point_term_is_a_small_share_of_the_bar(cid, spec):
    c = sr.Case(**spec)
    b = br.Bar(c)
    assert np.array_equal(b.G, br.grad_out(c)) and b.G.dtype == np.float32
    share_w, share_f = b.shares()
    assert share_w <= br.MAX_SHARE and share_f <= br.MAX_SHARE, (share_w, share_f)
    # the sums' headroom: 2^46 per term, rows far below 2^16 pairs
    assert np.bincount(b.pw.j, minlength=c.inp_pos.shape[0]).max() < 1 << 16
    # the cruder bound n_j sum_{cell, o} |W| is NOT what the bar uses: it is above the one it uses on every element
    n_j = np.bincount(b.pw.j, minlength=c.inp_pos.shape[0]).astype(np.float64)
    crude = n_j[:, None] * np.abs(c.filt.astype(np.float64)).reshape(64, c.cin, c.cout).sum((0, 2))[None, :]
    Bg = float(np.abs(b.G.astype(np.float64)).max()) * max(1.0, abs(float(c.window_fac)))
    assert np.all(b.fixed_f <= crude * Bg * 2.0 ** -45 * (1 + 1e-12))
