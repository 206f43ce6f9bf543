"""CPU checks of the ragged EMD (ABI 2.24: dmcf_emd_ragged) and its Python surface (ops.emd / ops.emd_ragged and
losses.emd_loss with row splits): the exported symbols, the workspace query, every error return on a fake device address, and
the host-side refusals in their order, each before the library is asked for.  No device is touched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_emd_ragged_workspace_bytes", "dmcf_emd_ragged"]
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
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.dmcf_version() >= 22400


def _i64(values):
    return None if values is None else (ctypes.c_int64 * len(values))(*values)


def _splits(counts):
    rs = [0]
    for c in counts:
        rs.append(rs[-1] + c)
    return rs


def _ws(hip_lib, sizes):
    rs1, rs2 = _splits([n for n, _ in sizes]), _splits([m for _, m in sizes])
    return hip_lib.dmcf_emd_ragged_workspace_bytes(rs1[-1], _i64(rs1), rs2[-1], _i64(rs2), len(sizes))


def test_workspace_bytes(hip_lib):
    ws = hip_lib.dmcf_emd_ragged_workspace_bytes
    rs1, rs2 = [0, 70, 70, 100], [0, 5, 5, 80]
    good = ws(100, _i64(rs1), 80, _i64(rs2), 3)
    assert good > 0
    # 0 for everything dmcf_emd_ragged refuses
    assert ws(-1, _i64(rs1), 80, _i64(rs2), 3) == 0 and ws(100, _i64(rs1), -1, _i64(rs2), 3) == 0
    assert ws(100, _i64(rs1), 80, _i64(rs2), 0) == 0 and ws(100, _i64(rs1), 80, _i64(rs2), -1) == 0
    assert ws(100, _i64(rs1), 80, _i64(rs2), MAX_BATCH + 1) == 0
    assert ws(100, None, 80, _i64(rs2), 3) == 0 and ws(100, _i64(rs1), 80, None, 3) == 0
    assert ws(100, _i64([1, 70, 70, 100]), 80, _i64(rs2), 3) == 0 and ws(100, _i64([0, 70, 60, 100]), 80, _i64(rs2), 3) == 0
    assert ws(99, _i64(rs1), 80, _i64(rs2), 3) == 0 and ws(100, _i64(rs1), 81, _i64(rs2), 3) == 0
    assert ws((1 << 31) - 200, _i64([0, (1 << 31) - 200]), 1, _i64([0, 1]), 1) == 0  # (int32 indices)
    # five state arrays over the concatenated rows (three of xyz1's, two of xyz2's), the tables and the partials
    for sizes in ([(1, 1)], [(64, 64)], [(1000, 30)] * 7, [(2025, 2025)] * 16, [(0, 0), (5, 0), (0, 5)], [(0, 0)]):
        n, m = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
        got = _ws(hip_lib, sizes)
        assert got >= 4 * (3 * n + 2 * m) and got > 0, sizes
        assert got % 256 == 0
    # the partials follow every item's own plan: 256 rows over 256 columns are one chunk, over 2,560 columns ten chunks of
    # 256 rows each -- 9 x 256 more floats in each of the two partial arrays of passes A and C than the state arrays explain
    one, ten = _ws(hip_lib, [(256, 256)]), _ws(hip_lib, [(256, 2560)])
    assert ten - one >= 4 * (2 * (2560 - 256) + 2 * 9 * 256)
    # ... and the same points cut into more items of fewer chunks each need fewer partials, not the same
    assert _ws(hip_lib, [(256, 256)] * 10) < _ws(hip_lib, [(2560, 2560)])


def test_error_returns(hip_lib):
    L = hip_lib
    rs1, rs2 = [0, 70, 70, 100], [0, 5, 9, 80]  # (item 1 has an empty first set: legal, cost 0)
    n, m, B = rs1[-1], rs2[-1], 3
    nb = L.dmcf_emd_ragged_workspace_bytes(n, _i64(rs1), m, _i64(rs2), B)
    assert nb > 0
    p = ctypes.c_void_p(FAKE)

    def call(n_=n, m_=m, rs1_=rs1, rs2_=rs2, batch=B, x1=p, x2=p, cost=p, ws=p, nb_=nb):
        return L.dmcf_emd_ragged(x1, n_, _i64(rs1_), x2, m_, _i64(rs2_), batch, cost, ws, nb_, None)

    assert call(batch=-1) == EINVAL
    assert call(batch=MAX_BATCH + 1) == EINVAL
    assert call(rs1_=None) == EINVAL and call(rs2_=None) == EINVAL
    assert call(n_=-1) == EINVAL and call(m_=-1) == EINVAL
    big = (1 << 31) - 200  # (int32 indices; the splits agree with the total, so nothing else refuses the call)
    assert call(n_=big, rs1_=[0, 70, 70, big]) == EINVAL and call(m_=big, rs2_=[0, 5, 9, big]) == EINVAL
    # row splits are read and validated on the host: they start at 0, do not decrease, end at the row count
    assert call(rs1_=[1, 70, 70, 100]) == EINVAL
    assert call(rs1_=[0, 70, 60, 100]) == EINVAL and call(rs2_=[0, 9, 5, 80]) == EINVAL
    assert call(rs1_=[0, 70, 70, 99]) == EINVAL and call(rs2_=[0, 5, 9, 81]) == EINVAL
    assert call(cost=None) == EINVAL and call(ws=None) == EINVAL and call(x1=None) == EINVAL and call(x2=None) == EINVAL
    assert call(nb_=nb - 1) == EWORKSPACE and call(nb_=0) == EWORKSPACE
    # an item with one empty set passes validation (unlike the ragged nn_distance): the call goes on to the workspace check
    assert call(rs1_=[0, 0, 70, 100], nb_=0) == EWORKSPACE
    # nothing to do: DMCF_OK with nothing enqueued and no pointer looked at (no device here to launch on)
    assert call(n_=0, m_=0, rs1_=[0, 0, 0, 0], rs2_=[0, 0, 0, 0], x1=None, x2=None, cost=None, ws=None, nb_=0) == OK
    assert call(n_=0, m_=0, rs1_=None, rs2_=None, batch=0, x1=None, x2=None, cost=None, ws=None, nb_=0) == OK
    assert call(batch=0, rs1_=None, rs2_=None) == EINVAL  # rows without an item


# ---- the Python surface ------------------------------------------------------------------------------------------------------
A5 = torch.zeros(5, 3)
B7 = torch.zeros(7, 3)
MALFORMED = [[1, 5], [0, 4], [0, 3, 2, 5], [5], [], [0, 1.5, 5]]  # (the list of tests/test_grid_pos_batched_abi.py)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test: the refusals below come before it is asked for."""
    from dmcf_amd import _lib

    def used():
        raise AssertionError("the library was asked for before the host-side checks were through")
    monkeypatch.setattr(_lib, "lib", used)


def test_signatures():
    from dmcf_amd import ops
    from dmcf_amd.utils.tools import losses
    assert list(inspect.signature(ops.emd).parameters) == ["xyz1", "xyz2", "n", "m", "row_splits1", "row_splits2"]
    assert list(inspect.signature(ops.emd_ragged).parameters) == ["xyz1", "xyz2", "row_splits1", "row_splits2"]
    assert list(inspect.signature(losses.emd_loss).parameters) == ["y_true", "y_pred", "n", "m", "true_row_splits",
                                                                   "pred_row_splits"]


def test_refusals_in_their_order(no_library):
    from dmcf_amd import ops
    from dmcf_amd.utils.tools.losses import emd_loss
    grad = A5.clone().requires_grad_(True)
    bad = [0, 4]
    # 1. one split alone -- whatever else is wrong with the call
    for kw in (dict(row_splits1=[0, 5]), dict(row_splits2=[0, 7]), dict(row_splits1=bad, n=[5]), dict(row_splits2=bad, m=[7])):
        with pytest.raises(NotImplementedError, match="both"):
            ops.emd(A5, B7, **kw)
        with pytest.raises(NotImplementedError, match="both"):
            ops.emd(grad, B7, **kw)
    with pytest.raises(NotImplementedError, match="both"):
        ops.emd_ragged(A5, B7, [0, 5], None)
    for kw in (dict(true_row_splits=[0, 5]), dict(pred_row_splits=[0, 7])):
        with pytest.raises(NotImplementedError, match="both"):
            emd_loss(A5, B7, **kw)
    # 2. splits together with counts -- before the gradient and the splits themselves are looked at
    for x, rs in ((A5, [0, 5]), (grad, [0, 5]), (A5, bad), (grad, bad)):
        for kw in (dict(n=[5]), dict(m=[7]), dict(n=5, m=7)):
            with pytest.raises(ValueError, match="not both"):
                ops.emd(x, B7, row_splits1=rs, row_splits2=[0, 7], **kw)
            with pytest.raises(ValueError, match="not both"):
                emd_loss(x, B7, true_row_splits=rs, pred_row_splits=[0, 7], **kw)
    # 3. no backward -- before the splits themselves are looked at
    for rs in ([0, 5], bad):
        with pytest.raises(NotImplementedError, match="backward"):
            ops.emd(grad, B7, row_splits1=rs, row_splits2=[0, 7])
        with pytest.raises(NotImplementedError, match="backward"):
            ops.emd_ragged(B7, grad, [0, 7], rs)
        with pytest.raises(NotImplementedError, match="backward"):
            emd_loss(B7, grad, true_row_splits=[0, 7], pred_row_splits=rs)


@pytest.mark.parametrize("bad", MALFORMED)
def test_malformed_row_splits_raise_before_the_device(no_library, bad):
    from dmcf_amd import ops
    from dmcf_amd.utils.tools.losses import emd_loss
    forms = [bad] + ([torch.tensor(bad, dtype=torch.int64)] if all(isinstance(v, int) for v in bad) else [])
    for rs in forms:
        with pytest.raises(ValueError):
            ops.emd(A5, B7, row_splits1=rs, row_splits2=[0, 2, 7])
        with pytest.raises(ValueError):
            ops.emd_ragged(B7, A5, [0, 2, 7], rs)
        with pytest.raises(ValueError):
            emd_loss(A5, B7, true_row_splits=rs, pred_row_splits=[0, 2, 7])


def test_unequal_lengths_shapes_and_the_forms_of_the_splits(no_library):
    from dmcf_amd import _lib, ops
    from dmcf_amd.utils.tools.losses import emd_loss
    with pytest.raises(ValueError, match="equal lengths"):
        ops.emd(A5, B7, row_splits1=[0, 2, 5], row_splits2=[0, 7])
    with pytest.raises(ValueError, match="equal lengths"):
        emd_loss(A5, B7, true_row_splits=[0, 5], pred_row_splits=[0, 3, 7])
    with pytest.raises(TypeError):
        ops.emd(A5, B7, row_splits1=torch.tensor([0, 5], dtype=torch.int32), row_splits2=[0, 7])
    with pytest.raises(TypeError):
        ops.emd_ragged(A5.numpy(), B7, [0, 5], [0, 7])
    with pytest.raises(ValueError, match="n_total"):  # the ragged form takes [n_total, 3] point sets
        ops.emd(A5.unsqueeze(0), B7.unsqueeze(0), row_splits1=[0, 5], row_splits2=[0, 7])
    # well-formed, items with one or both sets empty included, in every form the splits may take: on to the device check
    for rs1, rs2 in (([0, 2, 2, 5], [0, 3, 3, 7]), ([0, 0, 5], [0, 1, 7]), ([0, 5, 5], [0, 0, 7]),
                     (torch.tensor([0, 2, 5]), (0, 3, 7)), (ops.RowSplits([0, 5], None), np.array([0, 7]))):
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            ops.emd(A5, B7, row_splits1=rs1, row_splits2=rs2)
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            emd_loss(A5, B7, true_row_splits=rs1, pred_row_splits=rs2)
    with torch.no_grad(), pytest.raises(_lib.DmcfError, match="GPU only"):  # (under no_grad nothing wants a gradient)
        ops.emd(A5.clone().requires_grad_(True), B7, row_splits1=[0, 5], row_splits2=[0, 7])


class _Recording:
    """A stand-in for the library that records every entry point called with its arguments and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dmcf_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 512 if name.endswith("_workspace_bytes") else 0
        return entry


def test_emd_without_splits_is_unchanged(monkeypatch):
    """Without row splits ops.emd asks dmcf_emd_workspace_bytes and calls dmcf_emd once for the padded batch, with the counts it
    was given -- the calls and arguments it made before it took row splits -- and never the ragged entry point."""
    from dmcf_amd import _lib, ops
    stub = _Recording()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    monkeypatch.setattr(ops, "_pair_batch", lambda a, b: (a, b, True))  # (the device check of the operands, passed)
    a, b = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)

    def counts(p):
        return None if p is None else [p[i] for i in range(2)]

    for kw, c1, c2 in ((dict(), None, None), (dict(n=None, m=None, row_splits1=None, row_splits2=None), None, None),
                       (dict(n=[5, 2], m=torch.tensor([0, 7])), [5, 2], [0, 7]), (dict(n=3), [3, 3], None)):
        stub.calls.clear()
        cost = ops.emd(a, b, **kw)
        assert cost.shape == (2,) and cost.dtype == torch.float32
        (q, qa), (f, fa) = stub.calls  # exactly these two, in this order
        assert q == "dmcf_emd_workspace_bytes" and qa == (2, 5, 7)
        assert f == "dmcf_emd" and len(fa) == 11
        assert fa[0].value == a.data_ptr() and fa[1].value == b.data_ptr() and fa[2:5] == (2, 5, 7)
        assert counts(fa[5]) == c1 and counts(fa[6]) == c2
        assert fa[7].value == cost.data_ptr() and fa[8].value is not None and fa[9] == 512 and fa[10] == "the stream"
    stub.calls.clear()
    assert ops.emd(a, b, [5, 2], [7, 7]).shape == (2,)  # (n and m keep their positions)
    assert [name for name, _ in stub.calls] == ["dmcf_emd_workspace_bytes", "dmcf_emd"]
    assert counts(stub.calls[1][1][5]) == [5, 2] and counts(stub.calls[1][1][6]) == [7, 7]
