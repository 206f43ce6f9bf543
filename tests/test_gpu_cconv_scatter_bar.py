"""The scatter form of CConv (splat S: ops.scatter_plan + ops.cconv_scatter_forward) against the float64 reference, element by
element (tests/cconv_scatter_ref.py):

    |gpu - ref| <= (kbar * A + C_GEO * A1) * 2^-24 + n_i * B * 2^-45

on deterministic lattices with controlled transposed row lengths (0, 1, 2, 63 .. 65, 127 .. 129, 257) and block populations
(1, 8, 9, 15 .. 17, 31 .. 33, 65), an interior origin, strays beyond the plan's region, a scene far from the origin, reach 2 - 4,
CSR, padded and cut transposed lists, signed features, an outlier 2^10 times the rest, and the three instantiations.  Every case
first asserts the instantiation's name as ops.scatter_kernel_name gives it -- dmcf_cconv_scatter_kernel_name, which reads the
function the launch reads (sct_pick) -- against the case's own restatement (cconv_scatter_ref.expected_kernel).  The sums are
integers: the same call twice, a second plan, the two list forms and the three block sizes return the same bits.  The same cases run on the CPU in tests/test_cconv_scatter_ref_cpu.py, where the bar is
shown sound.  The worst err / bar per instantiation is printed by test_report_worst_ratio (run with -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_scatter_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

MATRIX = sr.matrix()
HDR_NCELLS, HDR_OVERFLOW, HDR_M, HDR_REACH = 10, 12, 13, 14  # SctHeader as int32 words (csrc/cconv_sct.hip)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Call:
    """The device operands of a case, and the call on a transposed list form and a plan."""

    def __init__(self, c, dev):
        from dmcf_amd import ops
        self.c, self.dev, self.ops = c, dev, ops
        self.W, self.Q, self.P, self.F = _t(c.filt, dev), _t(c.out_pos, dev), _t(c.inp_pos, dev), _t(c.feat, dev)
        self.bias = _t(c.bias_v, dev)

    def plan(self, m=None):
        return self.ops.scatter_plan(self.P, self.Q, self.c.voxel, self.c.radius, block_cells=m or self.c.m)

    def run(self, plan, form=None):
        c = self.c
        if (form or c.form) == "csr":
            lst = (c.t_idx, c.t_rs, None)
        else:
            lst = (c.p_idx, c.p_begin, c.p_cnt)
        t_idx, t_rb, t_cnt = (_t(x, self.dev) for x in lst)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        y = self.ops.cconv_scatter_forward(self.W, self.Q, c.extent, self.P, self.F, t_idx, t_rb, t_cnt, plan, window=c.window,
                                           window_fac=c.window_fac, bias=self.bias, out=_t(c.prior, self.dev),
                                           accumulate=c.prior is not None, error_flag=flag)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0, "a pair fell outside its block's box"
        return y.cpu().numpy()


def _header(plan):
    return plan.buf[:256].view(torch.int32).cpu().numpy()


def _populations(plan):
    """Points per block of the plan's table (cell_start follows the 256-byte header)."""
    n = int(_header(plan)[HDR_NCELLS])
    return np.diff(plan.buf[256:256 + 4 * (n + 1)].view(torch.int32).cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("cid,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_kernel_within_the_bar(dev, cid, spec):
    from dmcf_amd import ops
    c = sr.Case(**spec)
    assert ops.scatter_kernel_name(c.cout, c.m, c.reach) == c.kernel
    call = _Call(c, dev)
    plan = call.plan()
    hdr = _header(plan)
    assert (int(hdr[HDR_M]), int(hdr[HDR_REACH])) == (plan.block_cells, plan.reach) == (c.m, c.reach)
    pop = _populations(plan)
    assert set(sr.POPULATIONS) <= set(int(x) for x in pop), "the plan's blocks do not hold the populations the case builds"
    assert int(pop.sum()) + int(hdr[HDR_OVERFLOW]) == c.inp_pos.shape[0]
    if c.strays:
        assert int(hdr[HDR_OVERFLOW]) >= len(c.scene.strays) > 0, f"expected overflow rows, header says {hdr[HDR_OVERFLOW]}"
    else:
        assert int(hdr[HDR_OVERFLOW]) == 0
    if c.form == "cut":
        assert c.cut_rows.sum() >= 1, "no row cut off by the capacity"
    y = call.run(plan)
    exact = c.exact_rows_value()
    empty = c.n_pairs == 0
    assert empty.sum() >= len(sr.EMPTY_CELLS)
    assert np.array_equal(y[empty], exact[empty]), "a row without pairs is not exactly bias / prior content"
    if c.zero_channel is not None:  # a zero filter slice: exactly the bias (and the prior content)
        assert np.array_equal(y[:, c.zero_channel], exact[:, c.zero_channel])
    sr.check(c.kernel + (" two per CU" if c.cout == 8 and sr.two_workgroups(c.cout, c.m, c.reach) else ""), y, c)


@pytest.fixture(scope="module")
def identity(dev):
    c = sr.Case(**sr.IDENTITY)
    call = _Call(c, dev)
    plan = call.plan()
    return c, call, plan, call.run(plan)


def test_same_call_twice_same_bits(identity):
    c, call, plan, y = identity
    sr.check("identity", y, c)
    assert np.array_equal(y.view(np.int32), call.run(plan).view(np.int32))


def test_a_second_plan_same_bits(identity):
    """The orders inside a plan come out of atomics; the sums are integers."""
    c, call, plan, y = identity
    assert np.array_equal(y.view(np.int32), call.run(call.plan()).view(np.int32))


def test_csr_and_padded_list_same_bits(identity):
    c, call, plan, y = identity
    assert c.form == "csr" and c.cut == 0
    assert np.array_equal(y.view(np.int32), call.run(plan, form="padded").view(np.int32))


def test_block_sizes_same_bits(identity):
    """block_cells 1, 2 and 4 (boxes of 10^3, 11^3 and 13^3 slots; 8 and 16 waves) on one case without accumulate."""
    from dmcf_amd import ops
    c, call, plan, y = identity
    assert c.prior is None
    names = set()
    for m in (1, 2, 4):
        names.add(ops.scatter_kernel_name(c.cout, m, c.reach))
        p = call.plan(m)
        assert int(_header(p)[HDR_M]) == m
        assert np.array_equal(y.view(np.int32), call.run(p).view(np.int32)), f"block_cells {m} gives other bits"
    assert names == {"cconv_sct_kernel<4, 8>", "cconv_sct_kernel<4, 16>"}


# ---- the wrapper: operands are checked before any pointer is taken; empty calls give the bias ----------------------------------------

def _operands(dev, n_out=5, n_inp=7, cin=3, cout=4, pairs=9):
    from dmcf_amd import ops
    g = torch.Generator().manual_seed(5)
    a = dict(filters=torch.rand(4, 4, 4, cin, cout, generator=g), out_positions=torch.rand(n_out, 3, generator=g),
             inp_positions=torch.rand(n_inp, 3, generator=g), inp_features=torch.rand(n_inp, cin, generator=g),
             t_index=torch.zeros(pairs, dtype=torch.int32), t_row_begin=torch.zeros(n_inp + 1, dtype=torch.int64),
             t_row_count=torch.zeros(n_inp, dtype=torch.int32), bias=torch.rand(cout, generator=g),
             error_flag=torch.zeros(1, dtype=torch.int32))
    a = {k: v.to(dev) for k, v in a.items()}
    # (a plan that was never built: a check that came after a pointer was taken would hand the library an empty buffer)
    plan = ops.ScatterPlan(torch.empty(0, dtype=torch.uint8, device=dev), 0.1, 4, 4, n_inp, ())
    return a, plan


def _call(a, plan, **kw):
    from dmcf_amd import ops
    return ops.cconv_scatter_forward(a["filters"], a["out_positions"], 0.8, a["inp_positions"], a["inp_features"], a["t_index"],
                                     a["t_row_begin"], a["t_row_count"], plan, window="poly6", bias=a["bias"],
                                     error_flag=a["error_flag"], **kw)


@pytest.mark.parametrize("name,bad", [
    ("t_index", lambda t: t.long()), ("t_index", lambda t: t.cpu()), ("t_index", lambda t: t.repeat(2)[::2]),
    ("t_row_begin", lambda t: t.int()), ("t_row_begin", lambda t: t.cpu()), ("t_row_begin", lambda t: t.repeat(2)[::2]),
    ("t_row_count", lambda t: t.long()), ("t_row_count", lambda t: t.cpu()), ("t_row_count", lambda t: t.repeat(2)[::2]),
    ("bias", lambda t: t.double()), ("bias", lambda t: t.cpu()), ("bias", lambda t: t.repeat(2)[::2]), ("bias", lambda t: t[:3]),
    ("bias", lambda t: t.repeat(2)),
    ("error_flag", lambda t: t.long()), ("error_flag", lambda t: t.cpu()), ("error_flag", lambda t: t.repeat(4)[::2]),
])
def test_wrapper_rejects_an_operand_it_cannot_pass_on(dev, name, bad):
    a, plan = _operands(dev)
    a[name] = bad(a[name])
    with pytest.raises(ValueError, match=name):
        _call(a, plan)


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("name,bad", [
    ("filters", lambda t: t[0]), ("inp_features", lambda t: t[:-1]), ("t_row_begin", lambda t: t[:-1]),
    ("t_row_count", lambda t: t[:-1]), ("out", lambda t: t.cpu()), ("out", lambda t: t.double()), ("out", lambda t: t[:-1]),
])
def test_wrapper_rejects_operands_that_disagree(dev, name, bad, empty):
    """Shapes that do not fit the point sets, and an out tensor elsewhere: ValueError before any pointer is taken, in a call
    with an empty list too (which would otherwise return the bias without looking)."""
    a, plan = _operands(dev, pairs=0 if empty else 9)
    kw = {}
    if name == "out":
        kw["out"] = bad(torch.zeros(5, 4, device=dev))
    else:
        a[name] = bad(a[name])
    if name == "t_row_begin":
        a["t_row_count"] = None  # (CSR: n_inp + 1 row splits)
    with pytest.raises(ValueError, match="out has" if name == "out" else name):
        from dmcf_amd import ops
        ops.cconv_scatter_forward(a["filters"], a["out_positions"], 0.8, a["inp_positions"], a["inp_features"], a["t_index"],
                                  a["t_row_begin"], a["t_row_count"], plan, window="poly6", bias=a["bias"], **kw)


def test_wrapper_rejects_the_plan_of_an_empty_set_in_a_call_that_is_not_empty(dev):
    """scatter_plan for no output points holds nothing; a later call with output points on the same inputs must not take it."""
    from dmcf_amd import ops
    a, _ = _operands(dev)
    plan = ops.scatter_plan(a["inp_positions"], a["out_positions"][:0], 0.1, 0.4)
    assert plan.buf.numel() == 0 and plan.n_inp == a["inp_positions"].shape[0]
    with pytest.raises(ValueError, match="plan"):
        _call(a, plan)


def test_wrapper_rejects_a_plan_made_for_another_reach(identity, dev):
    """A plan for the case's radius and a call whose extent reaches one cell further: ValueError on the host that names both
    reaches, before anything is launched (a fresh error flag stays 0); with the matching extent the same operands are within
    the bar."""
    from dmcf_amd import ops
    c, call, plan, y = identity
    extent = 2.0 * (c.radius + c.voxel)
    assert plan.reach == c.reach and ops.scatter_reach(extent / 2, c.voxel) == c.reach + 1
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match=rf"reach of {c.reach} .* reach of {c.reach + 1}\b"):
        ops.cconv_scatter_forward(call.W, call.Q, extent, call.P, call.F, _t(c.t_idx, dev), _t(c.t_rs, dev), None, plan,
                                  window=c.window, window_fac=c.window_fac, bias=call.bias, error_flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    sr.check("identity, matching extent", call.run(plan), c)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("what", ["n_out", "n_inp", "t_index"])
def test_empty_call_gives_the_bias(dev, what, accumulate):
    """No output points, no input points or an empty list: the bias (prior content + bias under accumulate) and no launch --
    the plan of an empty input set is made without the library too."""
    from dmcf_amd import ops
    a, plan = _operands(dev, **{"n_out": dict(n_out=0), "n_inp": dict(n_inp=0), "t_index": dict(pairs=0)}[what])
    if what != "t_index":
        plan = ops.scatter_plan(a["inp_positions"], a["out_positions"], 0.1, 0.4)
        assert plan.buf.numel() == 0 and plan.reach == 4 and plan.block_cells == ops.SCATTER_BLOCK_CELLS
    n_out = a["out_positions"].shape[0]
    prior = torch.rand(n_out, 4, device=dev) if accumulate else None
    want = a["bias"].expand(n_out, 4) if prior is None else prior + a["bias"]
    y = _call(a, plan, out=None if prior is None else prior.clone(), accumulate=accumulate)
    assert y.shape == (n_out, 4) and torch.equal(y, want)
    a["bias"] = None
    y = _call(a, plan, out=None if prior is None else prior.clone(), accumulate=accumulate)
    assert torch.equal(y, torch.zeros(n_out, 4, device=dev) if prior is None else prior)


def test_report_worst_ratio():
    """Prints the worst err / bar of every instantiation of this file (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in sr.WORST.items()})
