"""The row, list and scan primitives on the GPU at their grid caps and tile edges, against the plain references of
tests/primitive_edges_ref.py (whose docstring names the kernels, the caps and the bars; tests/test_primitive_edges_cpu.py
asserts on the CPU that every case meets the conditions it is named for).

A  invert_neighbors_list: exact comparison with np.argsort(kind="stable")
B  reduce_subarrays_sum within (ceil(len / 16) + 5) * 2^-24 * sum |v| per row of the float64 sum; neighbor_counts exact
C  the row splits of a search whose counts are known by construction (scan_counts_to_row_splits), exact
D  dense_forward within 4e-7 * (|x| |W| + |b| + |r|), element by element
E  farthest_point_sample index for index with the oracle, with ties across the register / workspace boundary; gather_point exact
F  cconv_backward with K * Cin * Cout above the 4096 x 256 elements one pass of its element-wise kernels covers
(G, the filter packers above their caps, are cases of tests/cconv_forward_ref.matrix().)

The worst err / bar of B and D is printed by test_report_worst_ratio (run with -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as bref  # noqa: E402
import primitive_edges_ref as pe  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # (a copy: the references' arrays are read-only)


# ---- A ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pe.INVERT_CASES))
def test_invert_is_the_stable_argsort(dev, name):
    """pair_index[:m] is the stable order of the valid pairs by input, neighbors_index[:m] = rows[order],
    neighbors_attributes[:m] = attr[order], neighbors_row_splits = [0, cumsum(bincount(j, minlength=n_inp))], and every entry
    of neighbors_index and pair_index past m is -1 -- invalid entries (-1, n_inp, 2^31 - 1), padding slots and the slack of a
    buffer longer than its rows all land there and disturb no row.

    The list lengths sit either side of the sizes at which rocprim::radix_sort_pairs changes algorithm
    (rocprim/device/device_radix_sort.hpp):

        unsigned int single_sort_items_per_block
            = block_sort_config::block_size * block_sort_config::items_per_thread;
        if(size <= static_cast<decltype(size)>(single_sort_items_per_block))
        ...
        else if(static_cast<size_t>(size) <= merge_sort_limit && (sizeof(key_type) > 2 || size < 100000)

    a single-block sort up to 256 x 4 = 1024 items, a merge sort up to merge_sort_limit and onesweep above, with
    (rocprim/device/device_radix_sort_config.hpp)

        size_t MergeSortLimit  = 1024 * 1024>

    which is also the 4096 blocks x 256 threads invert_init and invert_gather cover in one pass.  The key widths sit either
    side of a power of two: the sentinel key n_inp then needs one bit more than the largest valid key."""
    from dmcf_amd import ops
    c = pe.invert_case(name)
    inv = ops.invert_neighbors_list(c["n_inp"], _t(c["index"], dev), _t(c["row_splits"], dev), _t(c["attr"], dev),
                                    neighbors_row_count=_t(c["row_count"], dev))
    torch.cuda.synchronize()
    P = c["index"].shape[0]
    assert inv.neighbors_index.shape == (P,) and inv.pair_index.shape == (P,) and inv.neighbors_row_splits.shape == (c["n_inp"] + 1,)
    attrs = inv.neighbors_attributes.cpu().numpy()
    assert attrs.shape == (P,)
    pe.check_invert(c, inv.neighbors_index.cpu().numpy(), inv.neighbors_row_splits.cpu().numpy(), attrs, inv.pair_index.cpu().numpy())


# ---- B ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rows,start", pe.REDUCE_CASES)
def test_reduce_subarrays_sum_and_neighbor_counts(dev, n_rows, start):
    from dmcf_amd import ops
    v, rs, ref, bar, lengths = pe.reduce_case(n_rows, start)
    got = ops.reduce_subarrays_sum(_t(v, dev), _t(rs, dev)).cpu().numpy()
    pe.check_reduce(got, ref, bar, lengths)
    cnt = ops.neighbor_counts(_t(rs, dev)).cpu().numpy()
    assert cnt.dtype == np.float32 and np.array_equal(cnt, np.diff(rs).astype(np.float32))


# ---- C ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", pe.SCAN_SIZES)
def test_search_row_splits_are_the_scan_of_the_counts(dev, m):
    from dmcf_amd import ops
    counts, want = pe.scan_expected(m)
    nns = ops.fixed_radius_search(_t(pe.scan_points(), dev), _t(pe.scan_queries(m), dev), pe.SCAN_RADIUS, return_distances=False)
    rs = nns.neighbors_row_splits.cpu().numpy()
    assert rs.dtype == np.int64 and np.array_equal(rs, want), "neighbors_row_splits is not [0, cumsum(counts)]"
    idx = nns.neighbors_index.cpu().numpy()[:int(want[-1])]
    assert idx.shape[0] == want[-1] and idx.min() >= 0 and idx.max() < pe.POINT_SITE.size
    assert np.array_equal(pe.POINT_SITE[idx], np.repeat(pe.scan_sites(m), counts)), "a row holds a point of another cluster"


# ---- D ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", pe.DENSE_KM)
@pytest.mark.parametrize("n", pe.DENSE_N)
def test_dense_forward_at_the_tile_and_grid_edges(dev, n, k, m):
    """dense_rows walks tiles of 16 rows, 4 waves per block on a grid capped at 2048 blocks: 131,072 rows per pass of
    ``tile += nwaves``; 131,073 rows take the loop twice, 262,147 three times.  The bar of test_dense_forward_against_float64."""
    from dmcf_amd import ops
    x, W, b, r, ref, scale = pe.dense_case(n, k, m)
    X, Wt = _t(x, dev), _t(W, dev)
    assert ops.dense_supported(X, Wt)
    y = ops.dense_forward(X, Wt).cpu().numpy()
    yb = ops.dense_forward(X, Wt, _t(b, dev), _t(r, dev)).cpu().numpy()
    assert y.shape == (n, m) and yb.shape == (n, m)
    pe.check_dense(y, yb, b, r, ref, scale)


# ---- E ---------------------------------------------------------------------------------------------------------------------------

def _fps(dev, p, m):
    from dmcf_amd import ops
    idx = ops.farthest_point_sample(m, _t(p, dev).unsqueeze(0))
    assert idx.shape == (1, m) and idx.dtype == torch.int32
    return idx[0].cpu().numpy()


@pytest.mark.parametrize("n", pe.FPS_SIZES)
def test_farthest_point_sample_at_the_thread_and_register_edges(oracle, dev, n):
    p = pe.fps_cloud(n)
    assert np.array_equal(_fps(dev, p, pe.FPS_SAMPLES), oracle.farthest_point_sample(pe.FPS_SAMPLES, p))


@pytest.mark.parametrize("kind,n", pe.FPS_TIES)
def test_farthest_point_sample_ties_across_registers_and_workspace(oracle, dev, kind, n):
    """Exact ties between a point held in registers (index < 8192) and one in the workspace array: copies 8192 apart (equal
    i & 511: the lower index wins), mirror images (the smaller i & 511 wins, here the workspace point), and a lattice whose
    corners tie with equal i & 511 on both sides of 8192."""
    p = pe.fps_tie_points(kind, n)
    assert np.array_equal(_fps(dev, p, pe.FPS_SAMPLES), oracle.farthest_point_sample(pe.FPS_SAMPLES, p))


@pytest.mark.parametrize("m,ch", pe.GATHER_CASES)
def test_gather_point_channels_and_block_edges(dev, m, ch):
    from dmcf_amd import ops
    feats, idx = pe.gather_case(m, ch)
    got = ops.gather_point(_t(feats, dev).unsqueeze(0), _t(idx, dev).unsqueeze(0))
    assert got.shape == (1, m, ch) and np.array_equal(got[0].cpu().numpy(), feats[idx])


# ---- F ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,sym_axis,cin,cout,accumulate", pe.BWD_CAP_CASES, ids=["plain", "symmetric", "plain_accumulate"])
def test_backward_past_the_element_cap(dev, shape, sym_axis, cin, cout, accumulate):
    """(4, 4, 4) with Cin 128 -> Cout 132: K * Cin * Cout = 1,081,344 > 4096 x 256, so cconv_bwd_filter_reduce and
    cconv_bwd_filter_store (plain) and cconv_bwd_expand (symmetric: the full kernel above the cap, the stored half below)
    take their grid-stride loop a second time; once accumulating into non-zero gradients, where an element visited twice
    shows.  The bars and the reference of tests/test_gpu_cconv_backward_sets.py."""
    from test_gpu_cconv_backward_sets import _same_set
    K, n_full, n_stored = pe.bwd_cap_counts(shape, sym_axis, cin, cout)
    assert bref.bwd_supported(K, cin, cout)
    assert K * cin * cout > 4096 * 256
    sym = sym_axis is not None
    _same_set(pe.BWD_CAP_POINTS, pe.BWD_CAP_RADIUS, shape, cin, cout, 91 + sym, symmetric=sym, sym_axis=2 if not sym else sym_axis,
              accumulate=accumulate, tag="cap_sym" if sym else ("cap_acc" if accumulate else "cap"))


def test_report_worst_ratio():
    """Prints the worst err / bar of B (reduce) and D (dense), and of the backward cases of F (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in pe.WORST.items()},
          {k: round(v, 4) for k, v in bref.WORST.items() if k.startswith("cap")})
