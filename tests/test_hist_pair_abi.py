"""CPU checks of the velocity-histogram entry point (ABI 2.26: dmcf_hist_pair_ragged) and its host side: the exported symbols,
every error return on a fake device address, ops.percentile_plan against the installed numpy's np.percentile bit for bit, and
evaluation_helper._kl_from_counts against compare_dist.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import hist_pair_ref as ref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_hist_pair_ragged_workspace_bytes", "dmcf_hist_pair_ragged"]
OK, EINVAL, EWORKSPACE = 0, -1, -2
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it
MAX_BATCH = 1 << 26


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_exported_declared_and_listed(hip_lib):
    from dmcf_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.dmcf_version() >= 22600
    assert int(re.search(r"#define\s+DMCF_HIST_TILE_ROWS\s+(\d+)", header).group(1)) == ops.HIST_TILE_ROWS
    assert ctypes.sizeof(_lib.HistPlan) == 32  # struct dmcf_hist_plan: int32 per, int32 rank[4], float gamma[2], int32 reserved


def _i64(values):
    return None if values is None else (ctypes.c_int64 * len(values))(*values)


def _plan(counts, bin_size=25):
    """The plan ops.hist_pair_ragged writes for items of these sizes -> (plan array, bins_total)."""
    from dmcf_amd import _lib, ops
    plan, bins = (_lib.HistPlan * len(counts))(), 0
    for b, cnt in enumerate(counts):
        per = int((cnt // bin_size) ** (1 / 3))
        k5, k5n, g5 = ops.percentile_plan(cnt, 5)
        k95, k95n, g95 = ops.percentile_plan(cnt, 95)
        plan[b].per = per
        plan[b].rank[:] = [k5, k5n, k95, k95n]
        plan[b].gamma[:] = [g5, g95]
        bins += (per + 1) ** 3
    return plan, bins


def test_workspace_bytes(hip_lib):
    ws = hip_lib.dmcf_hist_pair_ragged_workspace_bytes
    good = ws(2025 * 16, 16, 125 * 16)
    # per item the [3 axes][4 targets][256] digit counters and the selection state, then the item and tile tables
    assert good >= 16 * (3 * 4 * 256 * 4 + 96) and good % 256 == 0
    assert ws(1, 1, 1) > 0
    assert ws(100, 0, 1) == 0 and ws(100, -1, 1) == 0 and ws(1 << 27, MAX_BATCH + 1, 1 << 27) == 0
    assert ws(-1, 1, 1) == 0 and ws(2, 3, 3) == 0  # (fewer rows than items: some item is empty)
    assert ws((1 << 31) - 257, 1, 1) == 0 and ws((1 << 31) - 258, 1, 1) > 0  # (int32 indices)
    assert ws(100, 1, 0) == 0 and ws(100, 2, 1) == 0 and ws(100, 1, 1 << 30) == 0  # (a bin per item; 2 bins_total in int32)
    assert ws(1 << 20, 1, 1) > ws(1 << 10, 1, 1)  # (the tile table grows with the rows)


def test_error_returns(hip_lib):
    L = hip_lib
    counts = [70, 1, 2025]
    rs = [0, 70, 71, 2096]
    plan, bins = _plan(counts)
    assert bins == 8 + 1 + 125
    n, B = rs[-1], 3
    nb = L.dmcf_hist_pair_ragged_workspace_bytes(n, B, bins)
    assert nb > 0
    p = ctypes.c_void_p(FAKE)

    def call(n_=n, rs_=rs, batch=B, plan_=plan, bins_=bins, x=p, y=p, pct=p, cnt=p, ws=p, nb_=nb):
        return L.dmcf_hist_pair_ragged(x, y, n_, _i64(rs_), batch, plan_, bins_, pct, cnt, ws, nb_, None)

    assert call(batch=0) == EINVAL and call(batch=-1) == EINVAL and call(batch=MAX_BATCH + 1) == EINVAL
    assert call(n_=-1) == EINVAL and call(rs_=None) == EINVAL and call(plan_=None) == EINVAL
    big = (1 << 31) - 257  # (int32 indices; the splits agree with the total, so nothing else refuses the call)
    assert call(n_=big, rs_=[0, 70, 71, big]) == EINVAL
    # row splits are read and validated on the host: they start at 0, do not decrease, end at the row count; no empty item
    assert call(rs_=[1, 70, 71, 2096]) == EINVAL and call(rs_=[0, 71, 70, 2096]) == EINVAL and call(rs_=[0, 70, 71, 2095]) == EINVAL
    assert call(rs_=[0, 70, 70, 2096]) == EINVAL
    # the plan is validated against the sizes: per, the four ranks (< 2 cnt), the weights, the sum of the bins
    for field, k, value in (("per", None, -1), ("per", None, 1024), ("rank", 0, -1), ("rank", 3, 140), ("rank", 1, 1 << 30),
                            ("gamma", 0, -0.25), ("gamma", 1, 1.5), ("gamma", 0, float("nan"))):
        bad, _ = _plan(counts)
        if k is None:
            setattr(bad[0], field, value)
        else:
            getattr(bad[0], field)[k] = value
        assert call(plan_=bad) == EINVAL, (field, k, value)
    assert call(bins_=bins - 1) == EINVAL and call(bins_=bins + 1) == EINVAL
    bad, _ = _plan(counts)
    bad[1].per = 1  # (8 bins where the total says 1)
    assert call(plan_=bad) == EINVAL
    for kw in (dict(x=None), dict(y=None), dict(pct=None), dict(cnt=None), dict(ws=None)):
        assert call(**kw) == EINVAL, kw
    assert call(nb_=nb - 1) == EWORKSPACE and call(nb_=0) == EWORKSPACE


# ---- the host plan -----------------------------------------------------------------------------------------------------------
def _both(cnt, kind, rng):
    """[2 cnt] float32 values: ``random``, or ``ties`` -- a few distinct values, so the neighbours of most ranks are equal."""
    if kind == "random":
        return (rng.random(2 * cnt, dtype=np.float32) - np.float32(0.5)) * np.float32(7.3)
    return rng.integers(-3, 4, size=2 * cnt).astype(np.float32) * np.float32(0.37)


def _check_plan(cnt, kind, rng):
    from dmcf_amd import ops
    both = _both(cnt, kind, rng)
    want = [np.percentile(both[:, None], q, axis=0)[0] for q in (5, 95)]
    plans = [ops.percentile_plan(cnt, q) for q in (5, 95)]
    part = np.partition(both, sorted({k for p in plans for k in p[:2]}))
    for (k, k_next, gamma), w, q in zip(plans, want, (5, 95)):
        assert 0 <= k <= k_next <= min(k + 1, 2 * cnt - 1) and isinstance(gamma, np.float32) and 0 <= gamma < 1
        got = ref.lerp(part[k], part[k_next], gamma)
        assert got.dtype == w.dtype == np.float32 and got.tobytes() == w.tobytes(), (cnt, kind, q, got, w, k, k_next, gamma)


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_percentile_plan_matches_numpy(kind):
    """lerp(sorted[k], sorted[k_next], gamma) from the plan, in numpy float32, IS np.percentile(both, q, axis=0) for float32
    data: this pins the installed numpy's arithmetic (the virtual index, its floor and the weight, all in float32), and fails
    if a numpy release changes it."""
    rng = np.random.default_rng(7)
    for cnt in range(1, 3001):
        _check_plan(cnt, kind, rng)


@pytest.mark.parametrize("cnt", [2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 1_000_003])
def test_percentile_plan_matches_numpy_where_float32_rounds_the_index(cnt):
    """2 cnt - 1 around 2^24 is not exact in float32, and neither is its product with the float32 quantile."""
    rng = np.random.default_rng(cnt)
    for kind in ("random", "ties"):
        _check_plan(cnt, kind, rng)


def test_percentile_plan_refuses_an_empty_set():
    from dmcf_amd import ops
    with pytest.raises(ValueError):
        ops.percentile_plan(0, 5)


# ---- the KL of given counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [((2000, 3), np.float32), ((1280, 3), np.float32), ((700, 2), np.float64), ((30, 3), np.float32)])
def test_kl_from_counts_matches_compare_dist(shape, dtype):
    """The four cases of tests/test_metrics_abi.py::test_compare_dist_matches_loop: numpy-built counts through _kl_from_counts
    give compare_dist's value bit for bit, in int64 and in the int32 the device writes."""
    from dmcf_amd.utils.evaluation_helper import _kl_from_counts, _kl_pairs, compare_dist
    rng = np.random.default_rng(shape[0])
    x = rng.normal(size=shape).astype(dtype)
    y = (rng.normal(size=shape) * 1.3 + 0.2).astype(dtype)
    for a, b in ((x, y), (y, x), (x, x)):
        _, ca, cb = ref.percentiles_and_counts(a, b)
        assert ca.sum() == cb.sum() == shape[0]
        want = compare_dist(a, b)
        assert _kl_from_counts(ca, cb) == want and _kl_from_counts(ca.astype(np.int32), cb.astype(np.int32)) == want
        kl_ab, kl_ba = _kl_pairs(np.concatenate([ca, cb, ca, cb]).astype(np.int32), [0, 2 * len(ca), 4 * len(ca)])
        assert kl_ab.dtype == np.float64 and list(kl_ab) == [want, want] and list(kl_ba) == [compare_dist(b, a)] * 2


# ---- the Python surface: refusals before the library is asked for -----------------------------------------------------------
def test_host_side_refusals(monkeypatch):
    from dmcf_amd import _lib, ops

    def used():
        raise AssertionError("the library was asked for before the host-side checks were through")
    monkeypatch.setattr(_lib, "lib", used)
    a = torch.zeros(5, 3)
    for x, y in ((a, a), (a.numpy(), a), (a.double(), a.double()), (torch.zeros(5, 2), torch.zeros(5, 2))):
        with pytest.raises(ValueError):  # (not on the device, not a tensor, not float32, not [n, 3])
            ops.hist_pair_ragged(x, y)
