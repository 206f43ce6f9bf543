"""dmcf_hist_pair_ragged on the GPU against the host code it replaces: the percentiles against np.percentile under ==, the
integer histograms against the host's np.bincount exactly, and both KL values against evaluation_helper.compare_dist(x, y) and
compare_dist(y, x) bit for bit -- per item of one ragged batch and for every item alone.

Shapes, the smallest that can break it (T = ops.HIST_TILE_ROWS rows per workgroup):
  cnt 1, 2, 24, 25, 26, 199, 200, 675, 2025   per = 0 (one bin, the host divides by zero), 1 and 2 at both edges of cnt // 25
                                              and of the cube root, and the 2,025 points of the validation scenes (per = 4)
  cnt T - 1, T, T + 1, 2 T + 1                 both edges of a tile, three tiles of one item
  one batch of all of them                    items start in the middle of the tile table and of the counts
  all values equal                            every digit of every pass is shared; bin_w = 1e-6 / per
  40 % of the rows equal to one value         the tie straddles rank k of the 5th (axes 0, 2) and of the 95th (axis 1) percentile
  values that differ in their low 8 bits      the first three passes select nothing; the last decides
  mixed signs with -0.0 and +0.0              the 5th percentile lands on the zeros of both signs
  z = 0                                       a 2-D scene: one axis degenerate
  outliers far beyond both percentiles        both ends of the clip
All random data is seeded; the reference values are computed once per module."""
import numpy as np
import pytest

import hist_pair_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _items():
    from dmcf_amd import ops
    T = ops.HIST_TILE_ROWS
    rng = np.random.default_rng(11)
    items = []

    def add(name, x, y):
        items.append((name, np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)))

    for cnt in (1, 2, 24, 25, 26, 199, 200, 675, 2025, T - 1, T, T + 1, 2 * T + 1):
        add(f"random{cnt}", rng.normal(size=(cnt, 3)), rng.normal(size=(cnt, 3)) * 1.3 + 0.2)
    add("equal", np.full((200, 3), 0.7), np.full((200, 3), 0.7))
    x, y = rng.uniform(0, 1, size=(675, 3)), rng.uniform(0, 1, size=(675, 3))
    for v in (x, y):
        tied = rng.random(675) < 0.4
        v[tied] = (0.03, 0.97, 0.03)
    add("ties", x, y)
    low = lambda: (np.uint32(0x3F800000) | rng.integers(0, 256, size=(199, 3)).astype(np.uint32)).view(np.float32)  # noqa: E731
    add("low8", low(), low())

    def zeros():
        v = np.where(rng.random((200, 3)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        u = rng.random(200)
        v[u < 0.03] = -rng.uniform(1e-3, 2, size=(int((u < 0.03).sum()), 3))
        v[u > 0.93] = rng.uniform(1e-3, 2, size=(int((u > 0.93).sum()), 3))
        return v
    add("zeros", zeros(), zeros())
    x, y = rng.normal(size=(675, 3)), rng.normal(size=(675, 3)) * 0.8
    x[:, 2] = y[:, 2] = 0
    add("flat", x, y)
    x, y = rng.normal(size=(2025, 3)), rng.normal(size=(2025, 3)) + 0.1
    x[rng.random(2025) < 0.03] *= 1e4
    y[rng.random(2025) < 0.03] *= -3e3
    add("outliers", x, y)
    return items


def _splits(counts):
    rs = [0]
    for c in counts:
        rs.append(rs[-1] + c)
    return rs


@pytest.fixture(scope="module")
def runs():
    """The items, the host's values for each (np.percentile, np.bincount, compare_dist in both directions), the ragged call
    over all of them and the call on each alone -- computed once."""
    from dmcf_amd import ops
    from dmcf_amd.utils.evaluation_helper import compare_dist
    items = _items()
    want = []
    for _, x, y in items:
        pct, cx, cy = ref.percentiles_and_counts(x, y)
        with np.errstate(divide="ignore"):
            want.append(dict(pct=pct, cx=cx, cy=cy, kl_xy=compare_dist(x, y), kl_yx=compare_dist(y, x)))
    rs = _splits([len(x) for _, x, _ in items])
    X = torch.from_numpy(np.concatenate([x for _, x, _ in items])).to(DEV)
    Y = torch.from_numpy(np.concatenate([y for _, _, y in items])).to(DEV)
    ragged = ops.hist_pair_ragged(X, Y, rs)
    alone = [ops.hist_pair_ragged(X[rs[k]:rs[k + 1]], Y[rs[k]:rs[k + 1]]) for k in range(len(items))]
    return dict(items=items, want=want, rs=rs, X=X, Y=Y, ragged=ragged, alone=alone)


def _check_item(name, want, pct, counts):
    """One item's device results (numpy) against the host's."""
    from dmcf_amd.utils.evaluation_helper import _kl_from_counts
    bins = len(want["cx"])
    assert pct.dtype == np.float32 and pct.shape == (2, 3) and counts.dtype == np.int32 and counts.shape == (2 * bins,), name
    assert np.all(pct == want["pct"]), (name, pct, want["pct"])
    cx, cy = counts[:bins], counts[bins:]
    assert np.array_equal(cx, want["cx"]) and np.array_equal(cy, want["cy"]), name
    assert _kl_from_counts(cx, cy) == want["kl_xy"] and _kl_from_counts(cy, cx) == want["kl_yx"], name


def test_every_item_of_the_batch_has_the_hosts_bits(runs):
    pct, counts, offsets = runs["ragged"]
    assert pct.shape == (len(runs["items"]), 2, 3) and len(offsets) == len(runs["items"]) + 1 and offsets[0] == 0
    assert counts.shape == (offsets[-1],)
    pct, counts = pct.cpu().numpy(), counts.cpu().numpy()
    for k, ((name, x, _), want) in enumerate(zip(runs["items"], runs["want"])):
        assert offsets[k + 1] - offsets[k] == 2 * (int((len(x) // 25) ** (1 / 3)) + 1) ** 3
        _check_item(name, want, pct[k], counts[offsets[k]:offsets[k + 1]])


def test_every_item_alone_has_the_hosts_bits(runs):
    for (name, _, _), want, (pct, counts, offsets) in zip(runs["items"], runs["want"], runs["alone"]):
        assert offsets == [0, counts.shape[0]]
        _check_item(name + " alone", want, pct[0].cpu().numpy(), counts.cpu().numpy())


def test_the_cases_are_what_they_claim(runs):
    """The edge cases above do occur in the data: ties across the selected ranks, percentiles on a zero, both clip ends."""
    by_name = {name: (x, y, w) for (name, x, y), w in zip(runs["items"], runs["want"])}
    x, y, w = by_name["equal"]
    assert np.all(w["pct"] == np.float32(0.7)) and w["cx"][0] == w["cy"][0] == 200
    x, y, w = by_name["ties"]
    assert np.all(w["pct"][0, [0, 2]] == np.float32(0.03)) and w["pct"][1, 1] == np.float32(0.97)
    x, y, w = by_name["low8"]
    assert np.all(w["pct"] >= 1) and np.all(w["pct"] < 1 + 2.0 ** -15)
    x, y, w = by_name["zeros"]
    assert np.all(w["pct"][0] == 0) and np.signbit(np.concatenate((x, y))).any()
    x, y, w = by_name["flat"]
    assert w["pct"][0, 2] == 0 and w["pct"][1, 2] == 0
    x, y, w = by_name["outliers"]
    side = round(len(w["cx"]) ** (1 / 3))
    assert side == 5 and w["cx"][0] > 0 and w["cx"][-1] > 0 and w["cy"][0] > 0 and w["cy"][-1] > 0


def test_second_call_and_other_forms_of_the_splits(runs):
    """The same bits from a second call (the workspace's counters and the counts are reset by every call), from device splits
    and RowSplits, and with a stale value in every output."""
    from dmcf_amd import ops
    X, Y, rs = runs["X"], runs["Y"], runs["rs"]
    dev_rs = torch.tensor(rs, dtype=torch.int64, device=DEV)
    for splits in (rs, dev_rs, ops.RowSplits(rs, dev_rs), tuple(rs)):
        pct, counts, offsets = ops.hist_pair_ragged(X, Y, splits)
        assert offsets == runs["ragged"][2]
        assert torch.equal(pct, runs["ragged"][0]) and torch.equal(counts, runs["ragged"][1])
    # the y -> x direction shares the percentiles and swaps the two blocks of counts
    pct, counts, offsets = ops.hist_pair_ragged(Y, X, rs)
    assert torch.equal(pct, runs["ragged"][0])
    c, s = counts.cpu().numpy(), runs["ragged"][1].cpu().numpy()
    for k in range(len(offsets) - 1):
        a, b, mid = offsets[k], offsets[k + 1], (offsets[k] + offsets[k + 1]) // 2
        assert np.array_equal(c[a:mid], s[mid:b]) and np.array_equal(c[mid:b], s[a:mid])


def test_compare_dist_pair(runs):
    from dmcf_amd.utils.evaluation_helper import compare_dist_pair
    want_xy, want_yx = [w["kl_xy"] for w in runs["want"]], [w["kl_yx"] for w in runs["want"]]
    kl_xy, kl_yx = compare_dist_pair(runs["X"], runs["Y"], row_splits=runs["rs"])
    assert kl_xy.dtype == kl_yx.dtype == np.float64 and list(kl_xy) == want_xy and list(kl_yx) == want_yx
    # numpy inputs and one item without splits
    name, x, y = runs["items"][8]
    kl_xy, kl_yx = compare_dist_pair(x, y)
    assert list(kl_xy) == [want_xy[8]] and list(kl_yx) == [want_yx[8]]
    # another bin size: the host's per and the host's value
    from dmcf_amd.utils.evaluation_helper import compare_dist
    kl_xy, kl_yx = compare_dist_pair(x, y, bin_size=10)
    assert kl_xy[0] == compare_dist(x, y, bin_size=10) and kl_yx[0] == compare_dist(y, x, bin_size=10)


def test_value_errors(runs):
    from dmcf_amd import ops
    X, Y, rs = runs["X"], runs["Y"], runs["rs"]
    with pytest.raises(ValueError, match="no rows"):
        ops.hist_pair_ragged(X, Y, [0, 5, 5, rs[-1]])
    with pytest.raises(ValueError, match="no rows"):
        ops.hist_pair_ragged(X[:0], Y[:0])
    with pytest.raises(ValueError, match="equal shapes"):
        ops.hist_pair_ragged(X, Y[:-1], rs)
    for bad in (X.double(), X.cpu(), X[:, :2], X.reshape(-1), X.cpu().numpy()):
        with pytest.raises(ValueError, match="float32 device tensor"):
            ops.hist_pair_ragged(bad, bad)
    for splits in ([1, rs[-1]], [0, 7, 5, rs[-1]], [0, rs[-1] - 1], [0]):
        with pytest.raises(ValueError):
            ops.hist_pair_ragged(X, Y, splits)
