"""GPU checks of the backward of the lattice form (dmcf_lattice_conv_backward, ops.lattice_conv_backward) and of its autograd
node (ops.LatticeConvFunction).

The lattices are built by hand and registered with lattice.register_points: centre 0, voxels that are powers of two (0.125, and
0.25 for the coarse set), so every position and every difference of positions is exact in float32 -- the stencil form (nominal
offsets d * voxel) and the neighbour-list form (differences of rounded positions) then describe the same pairs with the same
geometry.  Reference: the float64 restatement tests/cconv_backward_ref.py on the explicit list of an ops.fixed_radius_search
over the same points, under the bar of tests/test_gpu_cconv_backward.py, element by element:

    |gpu - ref| <= 256 * 2^-24 * A        (A: the same gradient from the absolute values of every term; floor 1e-6 max A)

Second comparison: the HIP ops.cconv_backward on that list.  It meets the same bar against the same reference, so the two HIP
results may differ by at most twice the bar."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_BAR = 256          # (tests/test_gpu_cconv_backward.py)
SLAB_ROWS = 1024     # kLatSlab of csrc/cconv_lat_bwd.inc: rows of the output list per partial filter-gradient sum
FINE, COARSE = 0.125, 0.25


def _dev():
    return torch.device("cuda:0")


def _lattice(voxel, minp, dims, fill, seed, family):
    """(positions [n, 3] on the device, registered as a lattice) over a seeded fraction of the cells of a box."""
    from dmcf_amd import lattice
    rng = np.random.default_rng(seed)
    dx, dy, dz = dims
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    cells = np.stack([x.ravel() + minp[0], y.ravel() + minp[1], z.ravel() + minp[2]], 1)
    cells = cells[rng.uniform(size=cells.shape[0]) < fill]
    cells = cells[rng.permutation(cells.shape[0])]  # (point order is not cell order)
    pos = torch.from_numpy((cells * np.float64(voxel)).astype(np.float32)).to(_dev())
    lattice.register_points(pos, torch.zeros(3, device=_dev()), [voxel] * 3, family, box=(list(minp), list(dims)),
                            center_host=(0.0, 0.0, 0.0))
    return pos


class Case:
    """One layer call between two hand-built lattices: the operands of ops.lattice_conv and the float64 reference."""

    def __init__(self, inp, out, extent, cin, cout, ks=(4, 4, 4), window="poly6", seed=0):
        from dmcf_amd import lattice, ops
        self.P_in = _lattice(*inp, seed=seed + 1, family=("t", seed))
        self.P_out = self.P_in if out is None else _lattice(*out, seed=seed + 2, family=("t", seed))
        rng = np.random.default_rng(seed)
        self.n_in, self.n_out = self.P_in.shape[0], self.P_out.shape[0]
        self.feat = rng.normal(size=(self.n_in, cin)).astype(np.float32)
        self.filt = rng.uniform(-1, 1, size=(*ks, cin, cout)).astype(np.float32)
        self.G = rng.normal(size=(self.n_out, cout)).astype(np.float32)
        self.extent, self.window, self.ks = float(extent), window, ks
        lp = lattice.pair(self.P_in, self.P_out, self.extent)
        assert lp is not None
        self.lp = lp
        vmin, vdim, parts = lp.plan(ops, self.extent, _dev())
        assert not lp.cropped
        self.F = torch.from_numpy(self.feat).to(_dev())
        self.W = torch.from_numpy(self.filt).to(_dev())
        self.Gt = torch.from_numpy(self.G).to(_dev())
        self.vmin, self.vdim, self.parts = vmin, vdim, parts
        self.lin = lp.inp.lin(vmin, vdim)
        self.kw = dict(inp_step=int(lp.ratio) if lp.ratio >= 1 else 1, out_stride=1 if lp.ratio >= 1 else 2, parts=parts,
                       window=window)
        self.table, self.tmin, self.voxel = lp.out.table(), lp.out.minp, lp.inp.voxel

    def volume(self, F=None):
        return self.lp.inp.volume(self.F if F is None else F, self.vmin, self.vdim)

    def backward(self, G=None, table=None, **kw):
        from dmcf_amd import ops
        return ops.lattice_conv_backward(self.W, self.volume(), self.vmin, self.table if table is None else table, self.tmin,
                                         self.n_out, self.voxel, self.extent, self.Gt if G is None else G, **self.kw, **kw)

    def per_point(self, gv):
        return gv.reshape(-1, gv.shape[-1])[self.lin]

    def reference(self):
        """float64 (d filters, d features), their bounds A, and the HIP neighbour-list backward on the same explicit list."""
        from dmcf_amd import ops
        radius = float(np.float32(0.5) * np.float32(self.extent))
        nns = ops.fixed_radius_search(self.P_in, self.P_out, radius, return_distances=True)
        idx, rs = nns.neighbors_index, nns.neighbors_row_splits
        pw = ref.PairWeights(self.P_out.cpu().numpy(), self.P_in.cpu().numpy(), idx.cpu().numpy(), rs.cpu().numpy(), self.extent,
                             list(self.ks), window=self.window)
        rw, rf, _ = ref.grads(pw, self.filt, self.feat, self.G)
        aw, af, _ = ref.grads(pw, self.filt, self.feat, self.G, abs_mode=True)
        hw, hf = ops.cconv_backward(self.W, self.P_out, self.extent, self.P_in, self.F, idx, rs, self.Gt,
                                    neighbors_value=nns.neighbors_distance, window=self.window)
        return (rw, rf), (aw, af), (hw.cpu().numpy(), hf.cpu().numpy()), int(idx.shape[0])

    def check(self, tag):
        gv, gw = self.backward()
        torch.cuda.synchronize()
        got = (gw.cpu().numpy(), self.per_point(gv).cpu().numpy())
        want, bound, hip, pairs = self.reference()
        assert pairs > 0
        # every cell of the volume without a point is a sum over the same pairs with no feature behind it: nothing reads it,
        # but it must be finite, and exactly zero where no output reaches
        assert torch.isfinite(gv).all()
        for k, name in enumerate(("filters", "features")):
            ref.check(f"lattice:{tag}:{name}", got[k], want[k], bound[k], K_BAR)
            ref.check(f"lattice-vs-list:{tag}:{name}", got[k], hip[k].astype(np.float64), 2.0 * bound[k], K_BAR)
        return gv, gw


SAME_BOX = ((-3, 2, -1), (21, 6, 5))  # two 16-row tiles along x with a ragged tail; compaction crosses the holes


@pytest.mark.parametrize("cin,cout", [(4, 3), (8, 16), (4, 20), (8, 32)])
@pytest.mark.parametrize("window", ["poly6", "cubic"])
def test_same_lattice(cin, cout, window):
    case = Case((FINE, *SAME_BOX, 0.7), None, 0.6, cin, cout, window=window, seed=cin * 100 + cout)
    assert case.lp.ratio == 1 and case.parts is None
    from dmcf_amd import ops
    assert ops.lattice_offsets(case.voxel, 0.3, _dev()).shape[0] == 57  # 57 mod 4 = 1: a ragged group of offsets
    case.check(f"same:{cin}x{cout}:{window}")


def test_same_lattice_3x3x3_filter():
    Case((FINE, *SAME_BOX, 0.7), None, 0.6, 8, 16, ks=(3, 3, 3), seed=5).check("same:3x3x3")


def test_outputs_coarser():
    case = Case((FINE, (-3, 2, -1), (21, 6, 5), 0.7), (COARSE, (-2, 1, -1), (11, 3, 3), 0.7), 0.6, 8, 16, seed=11)
    assert case.lp.ratio == 2 and case.kw["inp_step"] == 2
    case.check("coarser")


def test_outputs_finer_sum_over_parts():
    from dmcf_amd import ops
    case = Case((COARSE, (-2, 1, -1), (11, 3, 3), 0.7), (FINE, (-3, 2, -1), (21, 6, 5), 0.7), 1.2, 8, 16, seed=12)
    assert case.lp.ratio == 0.5 and len(case.parts) == 8
    gv, gw = case.check("finer")
    # grad_filters (and grad_volume) of the call = the sum of the single-part calls
    sw, sv = torch.zeros_like(gw).double(), torch.zeros_like(gv).double()
    for pt in case.parts:
        v1, w1 = ops.lattice_conv_backward(case.W, case.volume(), case.vmin, case.table, case.tmin, case.n_out, case.voxel,
                                           case.extent, case.Gt, **dict(case.kw, parts=[pt]))
        sw += w1.double()
        sv += v1.double()
    _, bound, _, _ = case.reference()
    ref.check("lattice:finer:sum-of-parts:filters", gw.cpu().numpy(), sw.cpu().numpy(), bound[0], K_BAR)
    ref.check("lattice:finer:sum-of-parts:features", case.per_point(gv).cpu().numpy(), case.per_point(sv).cpu().numpy(), bound[1], K_BAR)


def test_slab_reduction():
    case = Case((FINE, (0, 0, 0), (40, 16, 8), 0.9), None, 0.6, 8, 16, seed=21)
    assert (case.n_out + SLAB_ROWS - 1) // SLAB_ROWS >= 3
    case.check("slabs")


def test_degenerate_calls():
    case = Case((FINE, *SAME_BOX, 0.7), None, 0.6, 8, 16, seed=31)
    gv, gw = case.backward()
    # an all-empty table: no row, no gradient
    ev, ew = case.backward(table=torch.full_like(case.table, -1))
    assert not ev.any() and not ew.any()
    # grad_out = 0: exact zeros
    zv, zw = case.backward(G=torch.zeros_like(case.Gt))
    assert not zv.any() and not zw.any()
    # one output only: the bits of the combined call
    v_only, none = case.backward(need_filters=False)
    assert none is None and torch.equal(v_only, gv)
    none, w_only = case.backward(need_volume=False)
    assert none is None and torch.equal(w_only, gw)
    # no float atomics: the same call, the same bits
    gv2, gw2 = case.backward()
    assert torch.equal(gv, gv2) and torch.equal(gw, gw2)
    assert gw.abs().max() > 0 and gv.abs().max() > 0
    # cells no output reaches are zero: the volume is padded along x to whole 16-cell tiles, past the last output cell + reach
    from dmcf_amd import ops
    last = SAME_BOX[0][0] + SAME_BOX[1][0] - 1 + ops.lattice_reach(case.voxel, 0.3, _dev())[0] - case.vmin[0]
    assert last + 1 < gv.shape[2] and not gv[:, :, last + 1:].any()


def test_rows_outside_the_table_contribute_nothing():
    from dmcf_amd import ops
    case = Case((FINE, *SAME_BOX, 0.7), None, 0.6, 4, 20, seed=41)
    gv, gw = case.backward()
    extra = torch.cat([case.Gt, torch.full((5, case.Gt.shape[1]), 1.0e6, device=_dev())])
    v2, w2 = ops.lattice_conv_backward(case.W, case.volume(), case.vmin, case.table, case.tmin, case.n_out + 5, case.voxel,
                                       case.extent, extra, **case.kw)
    assert torch.equal(v2, gv) and torch.equal(w2, gw)


@pytest.mark.parametrize("which", ["same", "finer"])
def test_autograd(which):
    from dmcf_amd import ops
    if which == "same":
        case = Case((FINE, *SAME_BOX, 0.7), None, 0.6, 8, 16, seed=51)
    else:
        case = Case((COARSE, (-2, 1, -1), (11, 3, 3), 0.7), (FINE, (-3, 2, -1), (21, 6, 5), 0.7), 1.2, 4, 20, seed=52)
    gv, gw = case.backward()
    n_rows = case.n_out + 3  # three rows past the table: the forward leaves them alone, their grad_out reaches nothing
    G = torch.cat([case.Gt, torch.ones(3, case.Gt.shape[1], device=_dev())])
    W = case.W.clone().requires_grad_()
    F = case.F.clone().requires_grad_()
    bias = torch.randn(case.Gt.shape[1], device=_dev()).requires_grad_()
    plain = ops.lattice_conv(case.W, case.volume(), case.vmin, case.table, case.tmin, n_rows, case.voxel, case.extent,
                             bias=bias.detach(), **case.kw)
    assert plain.grad_fn is None
    out = ops.lattice_conv(W, case.volume(F), case.vmin, case.table, case.tmin, n_rows, case.voxel, case.extent, bias=bias, **case.kw)
    assert isinstance(out.grad_fn, ops.LatticeConvFunction._backward_cls)
    assert torch.equal(out, plain)  # recording changes nothing of the forward
    (out * G).sum().backward()
    assert torch.equal(W.grad, gw)
    assert torch.equal(F.grad, case.per_point(gv))  # the volume's indexing carries the gradient to the points
    # (a float32 sum of n terms in any order is within (n - 1) 2^-24 sum |x| of the exact one)
    exact = case.Gt.double().sum(0)
    assert ((bias.grad.double() - exact).abs() <= case.n_out * 2.0 ** -24 * case.Gt.double().abs().sum(0)).all()
    with pytest.raises(ValueError):
        ops.lattice_conv(W, case.volume(), case.vmin, case.table, case.tmin, n_rows, case.voxel, case.extent, out=plain,
                         accumulate=True, **case.kw)


def test_report_worst_ratio():
    """Prints the worst err / bar of every group above (DESIGN.md section 4.6 quotes the maximum)."""
    mine = {k: v for k, v in ref.WORST.items() if k.startswith("lattice")}
    for k in sorted(mine):
        print(f"{k}: worst err/bar {mine[k]:.3g}")
    assert all(v <= 1.0 for v in mine.values())
