"""CPU checks of the ragged EMD's gradient (ABI 2.25: dmcf_emd_ragged_with_levels, dmcf_emd_ragged_backward and its workspace
query) and of the recording Python surface (ops.emd_ragged_recording / emd_ragged_with_levels / emd_ragged_backward,
ops.nn_distance_ragged(record=True), losses.emd_loss_ragged, chamfer_loss with row splits, pipeline key train_set_losses): the
exported symbols, every error return on a fake device address, the host-side refusals in their order, the library calls a
recording call makes, and the split plans the GPU test's shapes were chosen for.  No device is touched."""
import ctypes
import inspect
import os
import re
import tempfile
import types

import pytest

torch = pytest.importorskip("torch")

from test_emd_ragged_abi import A5, B7, EINVAL, EWORKSPACE, FAKE, MALFORMED, MAX_BATCH, OK, _Recording, _i64, hip_lib, no_library  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_emd_ragged_with_levels", "dmcf_emd_ragged_backward_workspace_bytes", "dmcf_emd_ragged_backward"]


def test_symbols_exported_declared_and_listed(hip_lib):  # noqa: F811
    from dmcf_amd import _lib
    c = ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.dmcf_version() >= 22500
    # the argument lists of the header, as the loader declares them
    i64p = c.POINTER(c.c_int64)
    ragged = [c.c_void_p, c.c_int64, i64p, c.c_void_p, c.c_int64, i64p, c.c_int64]
    assert hip_lib.dmcf_emd_ragged_with_levels.argtypes == ragged + [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    assert hip_lib.dmcf_emd_ragged_with_levels.argtypes == hip_lib.dmcf_emd_ragged.argtypes[:8] + [c.c_void_p] + \
        hip_lib.dmcf_emd_ragged.argtypes[8:]  # (dmcf_emd_ragged's, plus levels after cost)
    assert hip_lib.dmcf_emd_ragged_backward_workspace_bytes.argtypes == hip_lib.dmcf_emd_ragged_workspace_bytes.argtypes
    assert hip_lib.dmcf_emd_ragged_backward_workspace_bytes.restype == c.c_size_t
    assert hip_lib.dmcf_emd_ragged_backward.argtypes == ragged + [c.c_void_p] * 5 + [c.c_size_t, c.c_void_p]
    for name, n_args in (("dmcf_emd_ragged_with_levels", 12), ("dmcf_emd_ragged_backward_workspace_bytes", 5),
                         ("dmcf_emd_ragged_backward", 14)):
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(decl.split(",")) == n_args == len(getattr(hip_lib, name).argtypes), name


RS1, RS2 = [0, 70, 70, 100], [0, 5, 9, 80]  # (item 1 has an empty first set: legal, zero gradients)
N, M, B = RS1[-1], RS2[-1], 3


def test_backward_workspace_bytes(hip_lib):  # noqa: F811
    ws = hip_lib.dmcf_emd_ragged_backward_workspace_bytes
    assert ws(N, _i64(RS1), M, _i64(RS2), B) > 0
    # 0 for everything dmcf_emd_ragged_backward refuses
    assert ws(-1, _i64(RS1), M, _i64(RS2), B) == 0 and ws(N, _i64(RS1), -1, _i64(RS2), B) == 0
    assert ws(N, _i64(RS1), M, _i64(RS2), 0) == 0 and ws(N, _i64(RS1), M, _i64(RS2), -1) == 0
    assert ws(N, _i64(RS1), M, _i64(RS2), MAX_BATCH + 1) == 0
    assert ws(N, None, M, _i64(RS2), B) == 0 and ws(N, _i64(RS1), M, None, B) == 0
    assert ws(N, _i64([1, 70, 70, 100]), M, _i64(RS2), B) == 0 and ws(N, _i64([0, 70, 60, 100]), M, _i64(RS2), B) == 0
    assert ws(N - 1, _i64(RS1), M, _i64(RS2), B) == 0 and ws(N, _i64(RS1), M + 1, _i64(RS2), B) == 0
    assert ws((1 << 31) - 200, _i64([0, (1 << 31) - 200]), 1, _i64([0, 1]), 1) == 0  # (int32 indices)

    def size(sizes):
        rs1, rs2 = [0], [0]
        for n, m in sizes:
            rs1.append(rs1[-1] + n)
            rs2.append(rs2[-1] + m)
        return ws(rs1[-1], _i64(rs1), rs2[-1], _i64(rs2), len(sizes))
    for sizes in ([(1, 1)], [(2025, 2025)] * 16, [(0, 0), (5, 0), (0, 5)], [(0, 0)]):
        assert size(sizes) > 0 and size(sizes) % 256 == 0, sizes
    # an item's partials are [nsplit, 3, rows] of its own plan: 256 rows over 2,560 columns are ten chunks, nine more than over
    # 256 columns -- 9 x 3 x 256 floats more, and ten 32-byte tile records instead of one
    assert size([(256, 2560)]) - size([(256, 256)]) >= 4 * 9 * 3 * 256
    # the two sides use the partials one after the other: the larger side sets the size
    assert size([(256, 2560)]) == size([(2560, 256)])
    # ... and the same points cut into more items of fewer chunks each need fewer partials
    assert size([(256, 256)] * 10) < size([(2560, 2560)])


def test_backward_error_returns(hip_lib):  # noqa: F811
    L = hip_lib
    nb = L.dmcf_emd_ragged_backward_workspace_bytes(N, _i64(RS1), M, _i64(RS2), B)
    assert nb > 0
    p = ctypes.c_void_p(FAKE)

    def call(n_=N, m_=M, rs1_=RS1, rs2_=RS2, batch=B, x1=p, x2=p, lv=p, gc=p, g1=p, g2=p, ws=p, nb_=nb):
        return L.dmcf_emd_ragged_backward(x1, n_, _i64(rs1_), x2, m_, _i64(rs2_), batch, lv, gc, g1, g2, ws, nb_, None)

    assert call(g1=None, g2=None) == EINVAL  # neither gradient wanted
    assert call(batch=-1) == EINVAL and call(batch=MAX_BATCH + 1) == EINVAL
    assert call(rs1_=None) == EINVAL and call(rs2_=None) == EINVAL
    assert call(n_=-1) == EINVAL and call(m_=-1) == EINVAL
    big = (1 << 31) - 200
    assert call(n_=big, rs1_=[0, 70, 70, big]) == EINVAL and call(m_=big, rs2_=[0, 5, 9, big]) == EINVAL
    assert call(rs1_=[1, 70, 70, 100]) == EINVAL
    assert call(rs1_=[0, 70, 60, 100]) == EINVAL and call(rs2_=[0, 9, 5, 80]) == EINVAL
    assert call(rs1_=[0, 70, 70, 99]) == EINVAL and call(rs2_=[0, 5, 9, 81]) == EINVAL
    # there is work: every input and the workspace are needed, whichever side is wanted
    for kw in (dict(x1=None), dict(x2=None), dict(lv=None), dict(gc=None), dict(ws=None)):
        assert call(**kw) == EINVAL, kw
        assert call(g1=None, **kw) == EINVAL and call(g2=None, **kw) == EINVAL, kw
    assert call(nb_=nb - 1) == EWORKSPACE and call(nb_=0) == EWORKSPACE
    assert call(g1=None, nb_=nb - 1) == EWORKSPACE and call(g2=None, nb_=0) == EWORKSPACE
    assert call(rs1_=[0, 0, 70, 100], nb_=0) == EWORKSPACE  # an item with one empty set passes validation
    # nothing to do and nothing to zero: DMCF_OK with no pointer but the splits looked at (no device here to launch on)
    none = dict(x1=None, x2=None, lv=None, gc=None, ws=None, nb_=0)
    assert call(n_=0, m_=0, rs1_=[0, 0, 0, 0], rs2_=[0, 0, 0, 0], **none) == OK
    assert call(n_=0, m_=0, rs1_=None, rs2_=None, batch=0, **none) == OK
    assert call(n_=0, m_=0, rs1_=[0, 0, 0, 0], rs2_=[0, 0, 0, 0], g1=None, g2=None, **none) == EINVAL
    assert call(batch=0, rs1_=None, rs2_=None) == EINVAL  # rows without an item


def test_with_levels_error_returns(hip_lib):  # noqa: F811
    L = hip_lib
    nb = L.dmcf_emd_ragged_workspace_bytes(N, _i64(RS1), M, _i64(RS2), B)
    p = ctypes.c_void_p(FAKE)

    def call(n_=N, m_=M, rs1_=RS1, rs2_=RS2, batch=B, x1=p, x2=p, cost=p, lv=p, ws=p, nb_=nb):
        return L.dmcf_emd_ragged_with_levels(x1, n_, _i64(rs1_), x2, m_, _i64(rs2_), batch, cost, lv, ws, nb_, None)

    assert call(lv=None) == EINVAL
    # ... and the refusals of dmcf_emd_ragged
    assert call(batch=-1) == EINVAL and call(batch=MAX_BATCH + 1) == EINVAL
    assert call(rs1_=None) == EINVAL and call(rs2_=None) == EINVAL and call(n_=-1) == EINVAL and call(m_=-1) == EINVAL
    assert call(rs1_=[1, 70, 70, 100]) == EINVAL and call(rs2_=[0, 9, 5, 80]) == EINVAL and call(rs1_=[0, 70, 70, 99]) == EINVAL
    assert call(cost=None) == EINVAL and call(ws=None) == EINVAL and call(x1=None) == EINVAL and call(x2=None) == EINVAL
    assert call(nb_=nb - 1) == EWORKSPACE and call(nb_=0) == EWORKSPACE
    # every item empty: DMCF_OK, nothing written (levels has no column then) and no pointer looked at
    assert call(n_=0, m_=0, rs1_=[0, 0, 0, 0], rs2_=[0, 0, 0, 0], x1=None, x2=None, cost=None, lv=None, ws=None, nb_=0) == OK
    assert call(n_=0, m_=0, rs1_=None, rs2_=None, batch=0, x1=None, x2=None, cost=None, lv=None, ws=None, nb_=0) == OK
    assert call(batch=0, rs1_=None, rs2_=None) == EINVAL


def test_the_plans_the_shapes_were_chosen_for():
    """mt_plan of csrc/metrics_plan.h restated (batch 1), checked against the header's constants: the gradient keeps every item's
    own plan, and (20000, 7000) has chunks of two tiles on both sides."""
    text = open(os.path.join(ROOT, "dmcf_amd", "csrc", "metrics_plan.h")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr \w+ (kMt\w+) = (\d+);", text)}
    assert const["kMtThreads"] == 256 and const["kMtTile"] == 256 and const["kMtTargetBlocks"] == 2048

    def plan(rows, cols):
        row_blocks, tiles = -(-rows // 256), max(-(-cols // 256), 1)
        ns = max(min(-(-2048 // row_blocks), tiles), 1)
        per = -(-tiles // ns)
        return row_blocks, -(-tiles // per), per * 256
    assert plan(20000, 7000) == (79, 14, 512) and plan(7000, 20000) == (28, 40, 512)
    assert plan(2025, 2025) == (8, 8, 256)
    assert plan(300, 700) == (2, 3, 256) and plan(700, 300) == (3, 2, 256)
    assert plan(256, 257) == (1, 2, 256) and plan(257, 256) == (2, 1, 256)
    assert plan(1, 1) == (1, 1, 256)


# ---- the Python surface --------------------------------------------------------------------------------------------------------
def test_signatures():
    from dmcf_amd import ops
    from dmcf_amd.utils.tools import losses
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    default = lambda f, k: inspect.signature(f).parameters[k].default  # noqa: E731
    assert params(ops.emd_ragged_recording) == params(ops.emd_ragged) == ["xyz1", "xyz2", "row_splits1", "row_splits2"]
    assert params(ops.emd_ragged_with_levels) == ["xyz1", "xyz2", "row_splits1", "row_splits2"]
    assert params(ops.emd_ragged_backward) == ["xyz1", "xyz2", "row_splits1", "row_splits2", "levels", "grad_cost", "need1", "need2"]
    assert params(ops.nn_distance_ragged) == ["xyz1", "xyz2", "row_splits1", "row_splits2", "want1", "want2", "record"]
    assert params(losses.emd_loss_ragged) == ["y_true", "y_pred", "true_row_splits", "pred_row_splits", "record"]
    assert params(chamfer_loss) == ["y_true", "y_pred", "true_row_splits", "pred_row_splits", "record"]
    for f in (ops.nn_distance_ragged, ops.emd_row_splits, ops.nn_distance_row_splits, losses.emd_loss_ragged, chamfer_loss):
        assert default(f, "record") is False, f  # recording is opt-in
    assert issubclass(ops.EmdRaggedFunction, torch.autograd.Function) and issubclass(ops.NnDistanceRaggedFunction, torch.autograd.Function)


def test_refusals_in_their_order_with_record(no_library):  # noqa: F811
    from dmcf_amd import _lib, ops
    from dmcf_amd.utils.tools.losses import emd_loss_ragged
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    grad = A5.clone().requires_grad_(True)
    bad = [0, 4]
    # 1. one split alone -- whatever else is wrong with the call, recording or not
    for x in (A5, grad):
        for rs1, rs2 in (([0, 5], None), (None, [0, 7]), (bad, None)):
            with pytest.raises(NotImplementedError, match="both"):
                ops.emd_ragged_recording(x, B7, rs1, rs2)
            with pytest.raises(NotImplementedError, match="both"):
                ops.nn_distance_ragged(x, B7, rs1, rs2, record=True)
            with pytest.raises(NotImplementedError, match="both"):
                emd_loss_ragged(x, B7, rs1, rs2, record=True)
    for kw in (dict(true_row_splits=[0, 5]), dict(pred_row_splits=[0, 7])):
        with pytest.raises(NotImplementedError, match="both"):
            chamfer_loss(grad, B7, record=True, **kw)
    # 2. without record a wanted gradient is still refused, before the splits themselves are looked at
    for rs in ([0, 5], bad):
        with pytest.raises(NotImplementedError, match="backward"):
            ops.nn_distance_ragged(grad, B7, rs, [0, 7])
        with pytest.raises(NotImplementedError, match="backward"):
            ops.nn_distance_ragged(grad, B7, rs, [0, 7], record=False)
        with pytest.raises(NotImplementedError, match="backward"):
            emd_loss_ragged(grad, B7, rs, [0, 7])
        with pytest.raises(NotImplementedError, match="backward"):
            chamfer_loss(B7, grad, true_row_splits=[0, 7], pred_row_splits=rs)
        with pytest.raises(NotImplementedError, match="backward"):
            ops.emd_row_splits((5, 3), (7, 3), rs, [0, 7], wants_grad=True)
        with pytest.raises(NotImplementedError, match="backward"):
            ops.nn_distance_row_splits((5, 3), (7, 3), rs, [0, 7], wants_grad=True)
    # 3. with record the same calls go on to the splits: malformed ones are a ValueError ...
    for x in (A5, grad):
        with pytest.raises(ValueError):
            ops.emd_ragged_recording(x, B7, bad, [0, 7])
        with pytest.raises(ValueError):
            ops.nn_distance_ragged(x, B7, bad, [0, 7], record=True)
        with pytest.raises(ValueError, match="equal lengths"):
            ops.emd_ragged_recording(x, B7, [0, 2, 5], [0, 7])
        with pytest.raises(ValueError, match="non-empty"):  # nn_distance: exactly one empty set
            chamfer_loss(x, B7, true_row_splits=[0, 5, 5], pred_row_splits=[0, 3, 7], record=True)
        with pytest.raises(ValueError, match="n_total"):
            ops.emd_ragged_recording(x.unsqueeze(0), B7.unsqueeze(0), [0, 5], [0, 7])
        # ... and well-formed ones reach the device check
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            ops.emd_ragged_recording(x, B7, [0, 5], [0, 7])
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            ops.nn_distance_ragged(x, B7, [0, 2, 5], [0, 3, 7], record=True)
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            emd_loss_ragged(x, B7, [0, 0, 5], [0, 1, 7], record=True)
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            chamfer_loss(x, B7, true_row_splits=[0, 5], pred_row_splits=[0, 7], record=True)
    assert ops.emd_row_splits((5, 3), (7, 3), [0, 5], [0, 7], wants_grad=True, record=True) == ((0, 5), (0, 7))
    assert ops.nn_distance_row_splits((5, 3), (7, 3), [0, 5], [0, 7], wants_grad=True, record=True) == ((0, 5), (0, 7))


@pytest.mark.parametrize("bad", MALFORMED)
def test_malformed_row_splits_raise_before_the_device(no_library, bad):  # noqa: F811
    from dmcf_amd import ops
    from dmcf_amd.utils.tools.losses import emd_loss_ragged
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    grad = A5.clone().requires_grad_(True)
    with pytest.raises(ValueError):
        ops.emd_ragged_recording(grad, B7, bad, [0, 2, 7])
    with pytest.raises(ValueError):
        ops.nn_distance_ragged(B7, grad, [0, 2, 7], bad, record=True)
    with pytest.raises(ValueError):
        emd_loss_ragged(grad, B7, bad, [0, 2, 7], record=True)
    with pytest.raises(ValueError):
        chamfer_loss(grad, B7, true_row_splits=bad, pred_row_splits=[0, 2, 7], record=True)
    with pytest.raises(ValueError):
        ops.emd_ragged_with_levels(A5, B7, bad, [0, 2, 7])
    with pytest.raises(ValueError):
        ops.emd_ragged_backward(A5, B7, [0, 2, 5], bad, torch.zeros(10, 12), torch.zeros(2))


def test_backward_operands_are_checked_before_the_library(no_library, monkeypatch):  # noqa: F811
    """ops.emd_ragged_backward: the sets, the splits, then levels and grad_cost (_dev_exact), each before the library."""
    from dmcf_amd import _lib, ops
    lv, gc = torch.zeros(10, 12), torch.zeros(1)
    with pytest.raises(TypeError):
        ops.emd_ragged_backward(A5.numpy(), B7, [0, 5], [0, 7], lv, gc)
    with pytest.raises(ValueError, match="n_total"):  # [n_total, 3] exactly: no batch axis, no 2-D sets
        ops.emd_ragged_backward(A5.unsqueeze(0), B7, [0, 5], [0, 7], lv, gc)
    with pytest.raises(ValueError, match="n_total"):
        ops.emd_ragged_backward(A5[:, :2], B7, [0, 5], [0, 7], lv, gc)
    with pytest.raises(NotImplementedError, match="both"):
        ops.emd_ragged_backward(A5, B7, [0, 5], None, lv, gc)
    with pytest.raises(ValueError, match="equal lengths"):
        ops.emd_ragged_backward(A5, B7, [0, 2, 5], [0, 7], lv, gc)
    with pytest.raises(_lib.DmcfError, match="GPU only"):
        ops.emd_ragged_backward(A5, B7, [0, 5], [0, 7], lv, gc)
    # past the device check of the sets (taken as passed): levels and grad_cost
    monkeypatch.setattr(ops, "_point_batch", lambda t, name: (t.unsqueeze(0), False))
    with pytest.raises(TypeError, match="levels"):
        ops.emd_ragged_backward(A5, B7, [0, 5], [0, 7], lv.numpy(), gc)
    with pytest.raises(_lib.DmcfError, match="levels"):
        ops.emd_ragged_backward(A5, B7, [0, 5], [0, 7], lv, gc)


def test_the_library_calls_of_a_recording_call(monkeypatch):
    """Nothing wants a gradient: the plain entry point, and never dmcf_emd_ragged_with_levels.  A wanted gradient: the recording
    forward once, with levels [10, n_total + m_total] after cost, and one dmcf_emd_ragged_backward call for the whole batch."""
    from dmcf_amd import _lib, ops
    stub = _Recording()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(ops, "_stream", lambda: "the stream")
    monkeypatch.setattr(ops, "_point_batch", lambda t, name: (t.unsqueeze(0), False))  # (the device check, taken as passed)
    monkeypatch.setattr(ops, "_dev_exact", lambda t, name, dtype, shape, device: t.contiguous())
    names = lambda: [name for name, _ in stub.calls]  # noqa: E731
    rs1, rs2 = [0, 2, 2, 5], [0, 3, 4, 7]
    grad = A5.clone().requires_grad_(True)
    for x, y in ((A5, B7), (A5.clone(), B7.clone())):
        stub.calls.clear()
        cost = ops.emd_ragged_recording(x, y, rs1, rs2)
        assert cost.shape == (3,) and cost.grad_fn is None
        assert names() == ["dmcf_emd_ragged_workspace_bytes", "dmcf_emd_ragged"]
    stub.calls.clear()
    with torch.no_grad():
        ops.emd_ragged_recording(grad, B7, rs1, rs2)
    assert names() == ["dmcf_emd_ragged_workspace_bytes", "dmcf_emd_ragged"]
    stub.calls.clear()
    cost = ops.emd_ragged_recording(grad, B7, rs1, rs2)
    assert cost.grad_fn is not None and names() == ["dmcf_emd_ragged_workspace_bytes", "dmcf_emd_ragged_with_levels"]
    fa = stub.calls[1][1]
    assert len(fa) == 12 and fa[1] == 5 and list(fa[2]) == rs1 and fa[4] == 7 and list(fa[5]) == rs2 and fa[6] == 3
    assert fa[7].value == cost.data_ptr() and fa[8].value is not None and fa[10] == 512 and fa[11] == "the stream"
    stub.calls.clear()
    cost.sum().backward()
    assert names() == ["dmcf_emd_ragged_backward_workspace_bytes", "dmcf_emd_ragged_backward"]
    q, fb = stub.calls[0][1], stub.calls[1][1]
    assert q[0] == 5 and list(q[1]) == rs1 and q[2] == 7 and list(q[3]) == rs2 and q[4] == 3
    assert len(fb) == 14 and fb[1] == 5 and list(fb[2]) == rs1 and fb[4] == 7 and list(fb[5]) == rs2 and fb[6] == 3
    assert fb[7].value == fa[8].value  # the recorded levels
    assert fb[9].value is not None and fb[10] is None  # only xyz1 wants a gradient
    assert fb[12] == 512 and fb[13] == "the stream"
    assert grad.grad.shape == (5, 3)
    # every item empty: zeros without a library call, recording or not
    stub.calls.clear()
    none = ops.emd_ragged_recording(grad[:0], B7[:0], [0, 0, 0], [0, 0, 0])
    assert none.shape == (2,) and not none.any() and names() == []


def test_train_set_losses_defaults_to_off_and_checks_its_names():
    from dmcf_amd.pipelines.simulator import SET_LOSSES, Simulator
    model = types.SimpleNamespace(loss_keys=lambda: ["weighted_mse"])
    make = lambda **kw: Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp(), **kw)  # noqa: E731
    assert SET_LOSSES == ("chamfer", "emd")
    for kw in (dict(), dict(train_batched=True), dict(train_set_losses=None), dict(train_batched=True, train_set_losses={})):
        sim = make(**kw)
        assert sim.set_losses == [] and sim.loss_keys() == ["weighted_mse"], kw
    sim = make(train_batched=True, train_set_losses={"emd": 0.1, "chamfer": 1})
    assert sim.set_losses == [("emd", 0.1), ("chamfer", 1.0)] and sim.loss_keys() == ["weighted_mse", "emd", "chamfer"]
    with pytest.raises(ValueError, match="hist"):
        make(train_batched=True, train_set_losses={"chamfer": 1.0, "hist": 1.0})
    with pytest.raises(ValueError, match="hist"):  # (an unknown name first, with or without train_batched)
        make(train_set_losses={"hist": 1.0})
    with pytest.raises(NotImplementedError, match="train_batched"):
        make(train_set_losses={"chamfer": 1.0})
    with pytest.raises(NotImplementedError, match="train_batched"):
        make(train_batched=False, train_set_losses={"emd": 1.0})
