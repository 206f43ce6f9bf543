"""CPU check of the blocked float64 reference of the CConv / ASCC backward (cconv_backward_ref.grads_blocked): the same
(d filters, d feats) and the same absolute-term bounds as the dense form (cconv_backward_ref.grads), to 1e-12 relative."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402


def _padded(idx, rs, stride, cut_rows):
    """The CSR list as padded rows of ``stride`` slots (garbage in the unused ones), the buffer cut so that the last
    ``cut_rows`` rows reach past it."""
    n_out = rs.shape[0] - 1
    counts = np.minimum(np.diff(rs), stride).astype(np.int32)
    pidx = np.full(n_out * stride, 987654, dtype=np.int32)
    pval = np.zeros(n_out * stride, dtype=np.float32)
    for i in range(n_out):
        pidx[i * stride:i * stride + counts[i]] = idx[rs[i]:rs[i] + counts[i]]
    begin = (np.arange(n_out + 1) * stride).astype(np.int64)
    cap = (n_out - cut_rows) * stride
    return pidx[:cap], begin, counts, pval[:cap]


CASES = [
    dict(name="distinct_more_outputs", n_out=500, n_inp=120),
    dict(name="distinct_more_inputs", n_out=90, n_inp=600, normalize=True),
    dict(name="padded_cut", n_out=300, n_inp=300, padded=True),
    dict(name="padded_cut_distinct", n_out=200, n_inp=350, padded=True, window="explicit"),
    dict(name="ascc_axis0", n_out=300, n_inp=300, symmetric=True, sym_axis=0),
    dict(name="ascc_axis1", n_out=300, n_inp=300, symmetric=True, sym_axis=1, window="peak"),
    dict(name="ascc_axis2_padded", n_out=300, n_inp=300, symmetric=True, sym_axis=2, padded=True),
    dict(name="normalize_importance", n_out=250, n_inp=400, normalize=True, imp=True, window="cubic"),
    dict(name="explicit", n_out=300, n_inp=300, window="explicit", imp=True),
    dict(name="no_window", n_out=300, n_inp=200, window=None),
    dict(name="axes_1_8_1", n_out=300, n_inp=300, shape=(1, 8, 1), dims=2),
    dict(name="axes_1_8_8", n_out=300, n_inp=250, shape=(1, 8, 8), dims=2, normalize=True),
    dict(name="ascc_1_8_8", n_out=300, n_inp=300, shape=(1, 8, 4), dims=2, symmetric=True, sym_axis=2),
]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_blocked_matches_dense(case, oracle):
    c = dict(case)
    rng = np.random.default_rng(len(c["name"]))
    n_out, n_inp = c["n_out"], c["n_inp"]
    sym = c.get("symmetric", False)
    inp = rng.uniform(0, 1, size=(n_inp, 3)).astype(np.float32)
    out = inp if sym else rng.uniform(0, 1.2, size=(n_out, 3)).astype(np.float32)
    if c.get("dims", 3) == 2:
        inp[:, 2] = 0.0
        out[:, 2] = 0.0
    radius = 0.15 if c.get("dims", 3) == 3 else 0.08
    extent = float(np.float32(2) * np.float32(radius))
    idx, rs, dist = oracle.fixed_radius_search(inp, out, radius, ignore_query_point=sym)
    row_count, nval = None, dist
    window = c.get("window", "poly6")
    if c.get("padded"):
        idx, rs, row_count, nval = _padded(idx, rs, 12, 5)
        window = "explicit" if window == "explicit" else window
        nval = None if window != "explicit" else nval
    if window == "explicit":
        nval = rng.uniform(0.1, 1.0, size=idx.shape[0]).astype(np.float32)
    shape = list(c.get("shape", (4, 4, 4)))
    full = list(shape)
    if sym:
        full[c["sym_axis"]] *= 2
    cin, cout = 3, 5
    filt = rng.uniform(-1, 1, size=(*shape, cin, cout)).astype(np.float32)
    feat = rng.normal(size=(n_inp, cin)).astype(np.float32)
    G = rng.normal(size=(n_out, cout)).astype(np.float32)
    imp = rng.uniform(0.2, 2.0, size=n_inp).astype(np.float32) if c.get("imp") else None
    pw = ref.PairWeights(out, inp, idx, rs, extent, full, window=window, nval=nval if window else None, inp_importance=imp,
                         row_count=row_count)
    if c.get("padded"):
        assert row_count[-5:].sum() > 0 and pw.i.max() < n_out - 5, "no row cut off by the capacity"
    if c["name"].startswith("distinct"):
        assert len(np.unique(pw.j)) < n_inp and len(np.unique(pw.i)) < n_out, "no unreferenced input or empty output row"
    kw = dict(normalize=c.get("normalize", False), symmetric=sym, sym_axis=c.get("sym_axis", 2))
    for abs_mode in (False, True):
        dw, df, _ = ref.grads(pw, filt, feat, G, abs_mode=abs_mode, **kw)
        # (a small block: many blocks per call, and cells split across them)
        bw, bf = ref.grads_blocked(pw, filt, feat, G, abs_mode=abs_mode, block_floats=4096, **kw)
        aw, af, _ = ref.grads(pw, filt, feat, G, abs_mode=True, **kw)
        assert bw.shape == dw.shape and bf.shape == df.shape
        assert np.all(np.abs(bw - dw) <= 1e-12 * (aw + 1e-300)), case["name"]
        assert np.all(np.abs(bf - df) <= 1e-12 * (af + 1e-300)), case["name"]
        if abs_mode:
            assert np.all(bw >= 0) and np.all(bf >= 0)


def test_plan_helper_chunks():
    """The helper's chunks tile the rows exactly, with the slab cap and the rows per slab of the kernel's loop."""
    for n_out, K, cin, cout in ((1, 64, 3, 5), (600, 64, 5, 7), (45000, 216, 32, 16), (40000, 64, 256, 4), (70000, 64, 1, 4)):
        pl = ref.bwd_plan(n_out, K, cin, cout)
        rows = [c[1] for c in pl["chunks"]]
        assert sum(rows) == n_out and all(r == pl["R"] for r in rows[:-1])
        for row0, r, rps, S in pl["chunks"]:
            assert 1 <= S <= pl["S"] <= ref.BWD_MAX_SLABS
            assert (S - 1) * rps < r <= S * rps
