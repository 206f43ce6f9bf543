"""The backward of the scatter form (ops.cconv_scatter_backward: dmcf_cconv_scatter_backward, csrc/cconv_sct_bwd.inc) on every
case of tests/cconv_scatter_ref.py -- transposed rows of 0, 1, 2, 63 .. 65, 127 .. 129 and 257 pairs, CSR / padded / cut lists, cin
1 .. 32, both couts, window None / poly6 with fac 0.5, the pair at the window's edge, strays, an offset of 60, a zero filter slice,
a feature outlier; n_inp is never a multiple of the 16-row chunk and 22 or 23 workgroups contribute partial filter gradients
(one chunk each: a 40003-particle case below makes every one of the 1024 workgroups walk two or three) --
against the float64 gradients of the forward list, element by element and with no row left out
(tests/cconv_scatter_backward_ref.py, whose CPU file shows the bar sound):

    |gpu - ref| <= 256 * 2^-24 * max(A, 1e-6 max A) + fixed

and against ops.cconv_backward on the forward list at twice the float part.  Rows without pairs are exactly zero, options that
skip one gradient leave the other's bits alone, calls repeat bit for bit, and ops.cconv_scatter_forward is a node of the graph.
The worst err / bar per group is printed by test_report_worst_ratio (run with -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_scatter_backward_ref as br  # noqa: E402
import cconv_scatter_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

MATRIX = sr.matrix()
CHUNK = 16  # kSbRows of csrc/cconv_sct_bwd.inc


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Call:
    """The device operands of a case and the call on its transposed list."""

    def __init__(self, c, dev, G):
        from dmcf_amd import ops
        self.c, self.dev, self.ops = c, dev, ops
        self.W, self.Q, self.P, self.F = _t(c.filt, dev), _t(c.out_pos, dev), _t(c.inp_pos, dev), _t(c.feat, dev)
        self.G = _t(G, dev)
        self.lst = tuple(_t(x, dev) for x in c.transposed())

    def run(self, **kw):
        c = self.c
        gw, gf = self.ops.cconv_scatter_backward(self.W, self.Q, c.extent, self.P, self.F, *self.lst, self.G, window=c.window,
                                                 window_fac=c.window_fac, **kw)
        return gw, gf

    def list_route(self):
        """ops.cconv_backward (dmcf_invert_neighbors_list + dmcf_cconv_backward) on the forward list of the same pairs."""
        c = self.c
        return self.ops.cconv_backward(self.W, self.Q, c.extent, self.P, self.F, _t(c.idx.astype(np.int32), self.dev), _t(c.rs, self.dev),
                                       self.G, window=c.window, window_fac=c.window_fac)


@pytest.mark.parametrize("cid,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_kernel_within_the_bar(dev, cid, spec):
    c = sr.Case(**spec)
    n_inp = c.inp_pos.shape[0]
    assert n_inp % CHUNK != 0 and n_inp > 2 * CHUNK  # a ragged last chunk, several workgroups
    b = br.Bar(c)
    call = _Call(c, dev, b.G)
    gw, gf = call.run()
    assert gw.shape == call.W.shape and gf.shape == call.F.shape
    gw_n, gf_n = gw.cpu().numpy(), gf.cpu().numpy()
    name = f"cconv_sct_bwd<{c.cout}>"
    b.check(name, gw_n, gf_n)
    # exactness: input points without pairs (rows cut off by the capacity included) get exactly zero
    lonely = np.bincount(b.pw.j, minlength=n_inp) == 0
    assert lonely.sum() >= 1
    if c.cut:
        assert c.cut_rows.sum() >= 1 and lonely[c.cut_rows].all(), "no row cut off by the capacity"
    assert not gf_n[lonely].any(), "a row without pairs is not exactly zero"
    if c.zero_channel is not None:
        # the gradient OF a zero filter slice is not zero -- it is what the reference gives (inside the check above) --, and
        # that output channel's grad_out reaches no feature gradient: dF is the same with that column of grad_out cleared
        z = c.zero_channel
        assert np.abs(b.want_w[..., z]).max() > 0 and np.abs(gw_n[..., z]).max() > 0
        G0 = b.G.copy()
        G0[:, z] = 0
        _, gf0 = _Call(c, dev, G0).run(need_filters=False)
        b.check(name + " zero slice", None, gf0.cpu().numpy())
    # the list route on the forward list of the same pairs: both meet the bar, so they differ by at most twice the float part
    lw, lf = call.list_route()
    b.check(name + " vs list", gw_n, gf_n, want_w=lw.double().cpu().numpy(), want_f=lf.double().cpu().numpy(), factor=2.0)
    # skipping one gradient leaves the other bit for bit
    w_only, none_f = call.run(need_features=False)
    none_w, f_only = call.run(need_filters=False)
    assert none_f is None and none_w is None
    assert torch.equal(w_only, gw) and torch.equal(f_only, gf)
    assert call.run(need_filters=False, need_features=False) == (None, None)


@pytest.fixture(scope="module")
def identity(dev):
    c = sr.Case(**sr.IDENTITY)
    b = br.Bar(c)
    call = _Call(c, dev, b.G)
    return c, b, call, call.run()


def test_same_call_twice_same_bits(identity):
    c, b, call, (gw, gf) = identity
    b.check("identity", gw.cpu().numpy(), gf.cpu().numpy())
    gw2, gf2 = call.run()
    assert torch.equal(gw, gw2) and torch.equal(gf, gf2)


def test_same_bits_on_another_stream_after_other_work(identity, dev):
    c, b, call, (gw, gf) = identity
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        junk = torch.rand(512, 512, device=dev)
        junk = (junk @ junk).sum()
        gw2, gf2 = call.run()
        gw3, gf3 = call.run()
    s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    assert torch.isfinite(junk)
    assert torch.equal(gw, gw2) and torch.equal(gf, gf2) and torch.equal(gw, gw3) and torch.equal(gf, gf3)


def test_csr_and_padded_list_same_bits(identity, dev):
    c, b, call, (gw, gf) = identity
    assert c.form == "csr" and c.cut == 0
    lst = tuple(_t(x, dev) for x in (c.p_idx, c.p_begin, c.p_cnt))
    gw2, gf2 = call.ops.cconv_scatter_backward(call.W, call.Q, c.extent, call.P, call.F, *lst, call.G, window=c.window,
                                               window_fac=c.window_fac)
    assert torch.equal(gw, gw2) and torch.equal(gf, gf2)


def test_scatter_forward_is_a_node_of_the_graph(identity, dev):
    from dmcf_amd import ops
    c, b, call, (gw, gf) = identity
    plan = ops.scatter_plan(call.P, call.Q, c.voxel, c.radius, block_cells=c.m)
    W = call.W.clone().requires_grad_()
    F = call.F.clone().requires_grad_()
    bias = _t(c.bias_v, dev).clone().requires_grad_()
    kw = dict(window=c.window, window_fac=c.window_fac)
    with torch.no_grad():
        plain = ops.cconv_scatter_forward(call.W, call.Q, c.extent, call.P, call.F, *call.lst, plan, bias=bias.detach(), **kw)
    out = ops.cconv_scatter_forward(W, call.Q, c.extent, call.P, F, *call.lst, plan, bias=bias, **kw)
    assert out.grad_fn is not None
    sr.check("recorded forward", out.detach().cpu().numpy(), c)
    # (the recorded call adds the bias after the kernel, the plain call inside its last launch: one rounding apart)
    assert torch.allclose(out.detach(), plain, rtol=0, atol=float(plain.abs().max()) * 2.0 ** -22)
    out.backward(call.G)
    assert torch.equal(W.grad, gw) and torch.equal(F.grad, gf)
    assert torch.equal(bias.grad, call.G.sum(0))
    # features alone
    F2 = call.F.clone().requires_grad_()
    out2 = ops.cconv_scatter_forward(call.W, call.Q, c.extent, call.P, F2, *call.lst, plan, **kw)
    assert out2.grad_fn is not None
    out2.backward(call.G)
    assert torch.equal(F2.grad, gf)
    with pytest.raises(ValueError, match="out="):
        ops.cconv_scatter_forward(W, call.Q, c.extent, call.P, call.F, *call.lst, plan, out=torch.zeros_like(plain), **kw)
    with pytest.raises(ValueError, match="out="):
        ops.cconv_scatter_forward(W, call.Q, c.extent, call.P, call.F, *call.lst, plan, out=torch.zeros_like(plain), accumulate=True, **kw)
    # the bias alone requires grad: still a node of the graph, as in ops.cconv_forward
    b2 = bias.detach().clone().requires_grad_()
    out3 = ops.cconv_scatter_forward(call.W, call.Q, c.extent, call.P, call.F, *call.lst, plan, bias=b2, **kw)
    assert out3.grad_fn is not None
    out3.backward(call.G)
    assert torch.equal(b2.grad, call.G.sum(0))
    # operands are checked before the node is made, as in a plain call
    with pytest.raises(ValueError, match="bias"):
        ops.cconv_scatter_forward(W, call.Q, c.extent, call.P, call.F, *call.lst, plan, bias=bias.detach()[:3], **kw)
    with pytest.raises(ValueError, match="error_flag"):
        ops.cconv_scatter_forward(W, call.Q, c.extent, call.P, call.F, *call.lst, plan, error_flag=torch.zeros(1, device=dev), **kw)
    # a list changed in place between forward and backward is an error, not another gradient
    lst = tuple(None if t is None else t.clone() for t in call.lst)
    W4 = call.W.clone().requires_grad_()
    out4 = ops.cconv_scatter_forward(W4, call.Q, c.extent, call.P, call.F, *lst, plan, **kw)
    lst[0].add_(0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out4.backward(call.G)
    # no grad mode, or nothing that requires grad: the call it always was
    with torch.no_grad():
        assert ops.cconv_scatter_forward(W, call.Q, c.extent, call.P, call.F, *call.lst, plan, **kw).grad_fn is None
    assert ops.cconv_scatter_forward(call.W, call.Q, c.extent, call.P, call.F, *call.lst, plan, **kw).grad_fn is None


# ---- more chunks than workgroups: every workgroup walks two or three chunks -----------------------------------------------------------

MAX_GROUPS = 1024  # kSbMaxGroups of csrc/cconv_sct_bwd.inc
N_MANY = 40003     # 2501 chunks of 16 rows, the last one ragged


@pytest.fixture(scope="module")
def many(dev):
    """40003 particles in a cube of edge 2.6 around the 11^3 points of a 0.2 lattice, R = 0.25 (about 1.5e5 pairs): the smallest
    kind of call in which a workgroup keeps its filter-gradient registers, its T tile and its integer sums over several chunks.
    Both lists come from the library's search (the neighbour set is symmetric); the constants of the pairs once, on the CPU."""
    from dmcf_amd import ops
    assert N_MANY > 2 * CHUNK * MAX_GROUPS and N_MANY % CHUNK != 0
    rng = np.random.default_rng(11)
    inp = rng.uniform(-1.3, 1.3, size=(N_MANY, 3)).astype(np.float32)
    ax = (np.arange(-5, 6) * 0.2).astype(np.float32)
    out = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    extent = float(np.float32(0.5))
    radius = float(np.float32(0.5) * np.float32(extent))
    P, Q = _t(inp, dev), _t(out, dev)
    fwd = ops.fixed_radius_search(P, Q, radius, return_distances=False)
    tr = ops.fixed_radius_search(Q, P, radius, return_distances=False)
    idx, rs = fwd.neighbors_index, fwd.neighbors_row_splits
    assert idx.shape[0] == tr.neighbors_index.shape[0] > 10 ** 5
    pw = br.ref.PairWeights(out, inp, idx.cpu().numpy(), rs.cpu().numpy(), extent, (4, 4, 4), window="poly6", f64=False)
    assert np.bincount(pw.j, minlength=N_MANY).min() == 0  # particles outside the lattice reach no point of it
    return dict(inp=inp, out=out, extent=extent, P=P, Q=Q, idx=idx, rs=rs, t_idx=tr.neighbors_index, t_rs=tr.neighbors_row_splits, pw=pw)


@pytest.mark.parametrize("cout", [4, 8])
def test_workgroups_that_walk_several_chunks(dev, many, cout):
    """The chunk loop's second and third turn: against the float64 gradients (blocked restatement) at the bar, against
    ops.cconv_backward on the forward list at twice its float part, and twice with the same bits."""
    import types
    from dmcf_amd import ops
    cin = 24
    rng = np.random.default_rng(100 + cout)
    n_out = many["out"].shape[0]
    filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
    feat = rng.normal(size=(N_MANY, cin)).astype(np.float32)
    # (uniform, not normal: the fixed-point term scales with max |G|, and a normal sample's maximum of 4 sigma pushed it past
    # the cap of 1 / 16 on the floor of the feature gradient's bar; the cap is a condition on the inputs, checked below)
    G = rng.uniform(-1, 1, size=(n_out, cout)).astype(np.float32)
    W, F, Gd = _t(filt, dev), _t(feat, dev), _t(G, dev)
    pw = many["pw"]

    def run():
        return ops.cconv_scatter_backward(W, many["Q"], many["extent"], many["P"], F, many["t_idx"], many["t_rs"], None, Gd, window="poly6")
    gw, gf = run()
    want_w, want_f = br.ref.grads_blocked(pw, filt, feat, G)
    A_w, A_f = br.ref.grads_blocked(pw, filt, feat, G, abs_mode=True)
    c = types.SimpleNamespace(window_fac=1.0, inp_pos=many["inp"], filt=filt, feat=feat, cin=cin, cout=cout)
    fixed_w, fixed_f = br.fixed_terms(c, pw, G)
    assert float(np.max(fixed_w / br.Bar.float_part(A_w))) <= br.MAX_SHARE and float(np.max(fixed_f / br.Bar.float_part(A_f))) <= br.MAX_SHARE
    lw, lf = ops.cconv_backward(W, many["Q"], many["extent"], many["P"], F, many["idx"], many["rs"], Gd, window="poly6")
    name = f"cconv_sct_bwd<{cout}> many chunks"
    for tag, got, want, other, A, fixed in (("filters", gw, want_w, lw, A_w, fixed_w), ("features", gf, want_f, lf, A_f, fixed_f)):
        got = got.double().cpu().numpy()
        for label, target, factor in ((name, want, 1.0), (name + " vs list", other.double().cpu().numpy(), 2.0)):
            bar = br.Bar.float_part(A, factor) + fixed
            err = np.abs(got - target)
            ratio = float(np.max(err / bar))
            br.WORST[f"{label}:{tag}"] = max(br.WORST.get(f"{label}:{tag}", 0.0), ratio)
            assert np.all(err <= bar), f"{label}:{tag}: worst err/bar {ratio:.3g} at {np.unravel_index(np.argmax(err / bar), err.shape)}"
    lonely = np.bincount(pw.j, minlength=N_MANY) == 0
    assert not gf.cpu().numpy()[lonely].any()
    gw2, gf2 = run()
    assert torch.equal(gw, gw2) and torch.equal(gf, gf2)


@pytest.mark.parametrize("what", ["n_out", "n_inp", "t_index"])
def test_empty_call_gives_zero_gradients(dev, what):
    from dmcf_amd import ops
    n_out, n_inp, pairs = (0 if what == "n_out" else 5), (0 if what == "n_inp" else 7), (0 if what == "t_index" else 9)
    W, Q, P, F = (torch.rand(4, 4, 4, 3, 4, device=dev), torch.rand(n_out, 3, device=dev), torch.rand(n_inp, 3, device=dev),
                  torch.rand(n_inp, 3, device=dev))
    idx, rs = torch.zeros(pairs, dtype=torch.int32, device=dev), torch.zeros(n_inp + 1, dtype=torch.int64, device=dev)
    gw, gf = ops.cconv_scatter_backward(W, Q, 0.8, P, F, idx, rs, None, torch.rand(n_out, 4, device=dev), window="poly6")
    assert gw.shape == W.shape and gf.shape == F.shape and not gw.any() and not gf.any()


@pytest.mark.parametrize("name,bad", [
    ("t_index", lambda t: t.long()), ("t_index", lambda t: t.cpu()), ("t_index", lambda t: t.repeat(2)[::2]),
    ("t_row_begin", lambda t: t.int()), ("t_row_begin", lambda t: t.cpu()), ("t_row_begin", lambda t: t[:-1]),
    ("t_row_count", lambda t: t.long()), ("t_row_count", lambda t: t[:-1]), ("inp_features", lambda t: t[:-1]),
    ("grad_out", lambda t: t[:-1]), ("filters", lambda t: t[0]),
])
def test_wrapper_rejects_an_operand_it_cannot_pass_on(dev, name, bad):
    from dmcf_amd import ops
    g = torch.Generator().manual_seed(5)
    a = dict(filters=torch.rand(4, 4, 4, 3, 4, generator=g), out_positions=torch.rand(5, 3, generator=g),
             inp_positions=torch.rand(7, 3, generator=g), inp_features=torch.rand(7, 3, generator=g),
             t_index=torch.zeros(9, dtype=torch.int32), t_row_begin=torch.zeros(8, dtype=torch.int64),
             t_row_count=torch.zeros(7, dtype=torch.int32), grad_out=torch.rand(5, 4, generator=g))
    a = {k: v.to(dev) for k, v in a.items()}
    a[name] = bad(a[name])
    if name == "t_row_begin":
        a["t_row_count"] = None
    with pytest.raises(ValueError, match=name):
        ops.cconv_scatter_backward(a["filters"], a["out_positions"], 0.8, a["inp_positions"], a["inp_features"], a["t_index"],
                                   a["t_row_begin"], a["t_row_count"], a["grad_out"], window="poly6")


def test_wrapper_refuses_other_windows(dev):
    from dmcf_amd import ops
    W, Q, P, F = torch.rand(4, 4, 4, 3, 4, device=dev), torch.rand(5, 3, device=dev), torch.rand(7, 3, device=dev), torch.rand(7, 3, device=dev)
    idx, rs = torch.zeros(9, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError):
        ops.cconv_scatter_backward(W, Q, 0.8, P, F, idx, rs, None, torch.rand(5, 4, device=dev), window="cubic")


def test_timer_record(identity):
    c, b, call, _ = identity
    ops = call.ops
    old = ops.timer
    ops.timer = ops.LaunchTimer()
    try:
        call.run()
        records = ops.timer.records
    finally:
        ops.timer = old
    assert [r[0] for r in records] == ["cconv_backward"] and records[0][1]["kernel"] == "cconv_sct_bwd"
    assert (records[0][1]["cin"], records[0][1]["cout"]) == (c.cin, c.cout)


def test_report_worst_ratio():
    """Prints the worst err / bar of every group of this file (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in br.WORST.items() if not k.startswith("restated")})
