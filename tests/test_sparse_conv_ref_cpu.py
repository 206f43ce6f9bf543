"""The float64 restatement of SparseConv / SparseConvTranspose (tests/sparse_conv_ref.py) checked against itself and against the
oracle's continuous_conv: what the GPU tests compare with has to be right first.  No GPU."""
import numpy as np
import pytest

import sparse_conv_ref as sr


def _odd(cases):
    return [c for c in cases if all(k % 2 for k in c.kernel_size)]


def test_case_margins():
    """Every pair is >= 0.15 voxel from the search threshold, every filter coordinate >= 0.2 from a half-integer, and the clamp
    never engages: pair sets and cells are the same in float32 and float64."""
    for c in sr.all_cases():
        thr, half, clamp = c.margins()
        assert thr >= 0.15 and half >= 0.2 and not clamp, (c.name, thr, half, clamp)
        idx, rs = c.conv_list
        assert idx.size > 0 and rs[-1] == idx.size
    assert any(np.any(c.offset != sr.default_offset(c.kernel_size)) and len(set(c.offset)) > 1 for c in sr.small_cases()), \
        "no case has an explicit offset that differs per axis"
    names = [c.name for c in sr.small_cases()]
    assert any(np.diff(c.conv_list[1]).min() == 0 for c in sr.small_cases()), "no case has an empty output row"
    assert len(set(names)) == len(names)


def test_forward_equals_oracle_continuous_conv_for_odd_kernels(oracle):
    for c in _odd(sr.small_cases()):
        idx, rs = c.conv_list
        got = oracle.continuous_conv(c.W, c.out, float(sr.extent(c.kernel_size, c.voxel)), c.inp, c.F, idx, rs,
                                     inp_importance=c.inp_importance, align_corners=False, coordinate_mapping="identity",
                                     interpolation="nearest_neighbor", normalize=c.normalize, f64=True)
        ref, A = c.forward(False)
        if c.bias is not None:
            got = got.astype(np.float64) + c.bias.astype(np.float64)
        # (the oracle returns its float64 sums rounded to float32: half an ulp of the result, far inside the bar)
        sr.check(got, ref, A, c.kbar(False), c.name)


def test_transpose_is_the_forward_with_the_flipped_kernel_for_odd_kernels():
    """SparseConvTranspose(W) = SparseConv(flip_zyx(W)) over the same pair set (normalisation and importances aside: they sit on
    different sides)."""
    for c in _odd(sr.small_cases()):
        W, F = c.W.astype(np.float64), c.F.astype(np.float64)
        tp, cp = c.transpose_pairs, c.conv_pairs
        one_t = sr.Pairs(tp.i, tp.j, tp.cell, np.ones(tp.i.size), tp.n_out, tp.n_inp)
        one_c = sr.Pairs(cp.i, cp.j, cp.cell, np.ones(cp.i.size), cp.n_out, cp.n_inp)
        a = sr.gather(one_t, W, F)
        b = sr.gather(one_c, W[::-1, ::-1, ::-1], F)
        assert np.allclose(a, b, rtol=0, atol=1e-12 * max(1.0, np.abs(a).max())), c.name


@pytest.mark.parametrize("k", [2, 3, 4])
def test_adjoint_identity(k):
    """<T_W f, g> = <f, S_{W^T} g>: the transpose from set A to set B with W is the adjoint of SparseConv from B to A with W
    transposed in its channel axes."""
    c = next(c for c in sr.small_cases() if c.kernel_size == [k, k, k])
    rng = np.random.default_rng(k)
    W = c.W.astype(np.float64)
    f = rng.normal(size=(c.inp.shape[0], c.cin))
    g = rng.normal(size=(c.out.shape[0], c.cout))
    tp = c.transpose_pairs
    Tf = sr.gather(sr.Pairs(tp.i, tp.j, tp.cell, np.ones(tp.i.size), tp.n_out, tp.n_inp), W, f)
    # SparseConv from B (c.out, the inputs now) to A (c.inp, the outputs now)
    idx, rs = sr.pair_sets(c.out, c.inp - c.shift(), c.radius)
    i = np.repeat(np.arange(c.inp.shape[0]), np.diff(rs))
    j = idx.astype(np.int64)
    cell = sr.cells(c.out[j].astype(np.float64) - c.inp[i], c.kernel_size, c.voxel, c.offset)
    Sg = sr.gather(sr.Pairs(i, j, cell, np.ones(i.size), c.inp.shape[0], c.out.shape[0]), np.swapaxes(W, 3, 4), g)
    lhs, rhs = (Tf * g).sum(), (f * Sg).sum()
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)), (lhs, rhs)


@pytest.mark.parametrize("transpose", [False, True])
def test_gradients_agree_with_central_differences(transpose):
    c = sr.small_cases()[1]  # k = 3, 5 -> 7, importance, normalize, bias, two inputs in one voxel
    (dW, _), (dF, _), (db, _), (dimp, _) = c.grads(transpose)
    G = c.G.astype(np.float64)
    imp_name = "out_importance" if transpose else "inp_importance"

    def loss(W=None, F=None, imp=None):
        import copy
        d = copy.copy(c)
        d.__dict__.pop("conv_pairs", None)
        d.__dict__.pop("transpose_pairs", None)
        if imp is not None:
            setattr(d, imp_name, imp)
        out = sr.gather(d.pairs(transpose), c.W.astype(np.float64) if W is None else W, c.F.astype(np.float64) if F is None else F)
        return (out * G).sum()

    rng = np.random.default_rng(0)
    h = 1e-5
    for _ in range(6):
        e = tuple(rng.integers(0, s) for s in c.W.shape)
        Wp, Wm = c.W.astype(np.float64), c.W.astype(np.float64)
        Wp[e] += h
        Wm[e] -= h
        assert abs((loss(W=Wp) - loss(W=Wm)) / (2 * h) - dW[e]) <= 1e-6 * max(1.0, abs(dW[e]))
        e = tuple(rng.integers(0, s) for s in c.F.shape)
        Fp, Fm = c.F.astype(np.float64), c.F.astype(np.float64)
        Fp[e] += h
        Fm[e] -= h
        assert abs((loss(F=Fp) - loss(F=Fm)) / (2 * h) - dF[e]) <= 1e-6 * max(1.0, abs(dF[e]))
        imp = getattr(c, imp_name).astype(np.float64)
        e = int(rng.integers(0, imp.shape[0]))
        ip, im = imp.copy(), imp.copy()
        ip[e] += h
        im[e] -= h
        assert abs((loss(imp=ip) - loss(imp=im)) / (2 * h) - dimp[e]) <= 1e-6 * max(1.0, abs(dimp[e]))
    assert np.allclose(db, G.sum(axis=0))
