"""CPU checks of the window sum with row splits (ABI 2.22: dmcf_frs_window_sum_batched, dmcf_frs_window_sum_backward_batched),
of its Python surface (ops.window_sum, losses.compute_density, losses.density_loss), of the pipeline key ``warm_up_batched``
and of the batched warm-up's exit bookkeeping on the host.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_frs_window_sum_batched", "dmcf_frs_window_sum_backward_batched"]
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -4
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it
IGNORE, O3D_CORNERS, O3D_WALK, LINF = 1, 2, 4, 8
W_NONE, W_POLY6, W_CUBIC_GRAD = 0, 2, 6


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
    assert hip_lib.dmcf_version() >= 22200


def test_signatures(hip_lib):
    """The un-batched argument lists with (row_splits, batch) after m, plus item_max before the stream for the forward."""
    c = ctypes
    L = hip_lib
    one = list(L.dmcf_frs_window_sum.argtypes)
    assert list(L.dmcf_frs_window_sum_batched.argtypes) == one[:2] + [c.c_void_p, c.c_int64] + one[2:-1] + [c.c_void_p, one[-1]]
    one = list(L.dmcf_frs_window_sum_backward.argtypes)
    assert list(L.dmcf_frs_window_sum_backward_batched.argtypes) == one[:2] + [c.c_void_p, c.c_int64] + one[2:]
    assert L.dmcf_frs_window_sum_batched.restype == c.c_int and L.dmcf_frs_window_sum_backward_batched.restype == c.c_int


def test_window_ids_match_the_header():
    from dmcf_amd import ops
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    for name, want in (("DMCF_WINDOW_NONE", W_NONE), ("DMCF_WINDOW_POLY6", W_POLY6), ("DMCF_WINDOW_CUBIC_GRAD", W_CUBIC_GRAD)):
        m = re.search(name + r"\s*=\s*(-?\d+)", text)
        assert m and int(m.group(1)) == want, name
    assert ops.WINDOWS[None] == W_NONE and ops.WINDOWS["cubic_grad"] == W_CUBIC_GRAD


def test_error_returns(hip_lib):
    L = hip_lib
    n, m, B = 100, 80, 3
    nb = L.dmcf_frs_workspace_bytes_batched(n, m, B)
    assert nb > 0
    q = rs = ws = out = mx = cq = cp = grad = ctypes.c_void_p(FAKE)

    def fwd(m_=m, rs_=rs, batch=B, flags=0, window=W_POLY6, ws_=ws, nb_=nb, out_=out, mx_=mx, q_=q, radius=0.1):
        return L.dmcf_frs_window_sum_batched(q_, m_, rs_, batch, n, radius, flags, window, ws_, nb_, out_, mx_, None)

    def bwd(m_=m, rs_=rs, batch=B, flags=0, window=W_POLY6, ws_=ws, nb_=nb, cq_=cq, cp_=cp, grad_=grad, q_=q, radius=0.1):
        return L.dmcf_frs_window_sum_backward_batched(q_, m_, rs_, batch, n, radius, flags, window, cq_, cp_, ws_, nb_, grad_, None)

    for call in (fwd, bwd):
        assert call(flags=16) == EINVAL and call(flags=IGNORE | 32) == EINVAL  # a flag other than IGNORE_QUERY_POINT
        assert call(flags=O3D_WALK) == EINVAL and call(flags=O3D_CORNERS) == EINVAL and call(flags=O3D_WALK | IGNORE) == EINVAL
        assert call(flags=LINF) == EUNSUPPORTED and call(flags=LINF | IGNORE) == EUNSUPPORTED
        for batch in (0, -1):
            assert call(batch=batch) == EINVAL
        assert call(rs_=None) == EINVAL
        assert call(window=W_NONE - 1) == EINVAL and call(window=W_CUBIC_GRAD + 1) == EINVAL
        assert call(ws_=None) == EINVAL
        assert call(radius=0.0) == EINVAL
        assert call(m_=-1) == EINVAL
        assert call(q_=None) == EINVAL
        assert call(nb_=nb - 1) == EWORKSPACE and call(nb_=1024) == EWORKSPACE
    assert fwd(out_=None) == EINVAL
    assert bwd(grad_=None) == EINVAL
    assert bwd(cq_=None, cp_=None) == EINVAL
    assert bwd(window=W_NONE) == EUNSUPPORTED
    assert fwd(window=W_CUBIC_GRAD) == EUNSUPPORTED  # item_max orders non-negative sums only
    # nothing to do: DMCF_OK with nothing launched (no device here to launch on)
    assert fwd(m_=0, mx_=None) == OK and fwd(m_=0, mx_=None, q_=None, out_=None) == OK
    assert bwd(m_=0) == OK and bwd(m_=0, q_=None, grad_=None) == OK
    # a coefficient array alone is enough for the backward's validation: it goes on to the workspace check
    assert bwd(cq_=None, nb_=nb - 1) == EWORKSPACE and bwd(cp_=None, nb_=nb - 1) == EWORKSPACE


P4 = torch.zeros(4, 3)
Q3 = torch.zeros(3, 3)
MALFORMED = [[1, 4], [0, 3], [0, 3, 2, 4], [4], [], [0, 1.5, 4]]  # (the list of tests/test_grid_pos_batched_abi.py)


def _poly6():
    from dmcf_amd.utils.tools import losses
    return losses.get_window_func("poly6")


def test_one_split_alone_raises():
    from dmcf_amd import ops
    from dmcf_amd.utils.tools import losses
    for kw in (dict(points_row_splits=[0, 4]), dict(queries_row_splits=[0, 3])):
        with pytest.raises(NotImplementedError):
            ops.window_sum(P4, Q3, 0.1, "poly6", **kw)
    with pytest.raises(NotImplementedError):
        ops.window_sum(P4, Q3, 0.1, "poly6", return_item_max=True)  # (the per-item maximum is the batched form's)
    for kw in (dict(out_row_splits=[0, 3]), dict(in_row_splits=[0, 4])):
        with pytest.raises(NotImplementedError):
            losses.compute_density(Q3, P4, 0.1, win=_poly6(), **kw)
    with pytest.raises(NotImplementedError):
        losses.compute_density(Q3, None, 0.1, win=_poly6(), in_row_splits=[0, 3])
    for kw in (dict(row_splits=[0, 3]), dict(in_row_splits=[0, 4])):
        with pytest.raises(NotImplementedError):
            losses.density_loss(Q3, Q3, P4, P4, 0.1, win=_poly6(), **kw)
    with pytest.raises(NotImplementedError):
        losses.density_loss(Q3, Q3, None, None, 0.1, win=_poly6(), in_row_splits=[0, 3])


@pytest.mark.parametrize("bad", MALFORMED)
def test_malformed_row_splits_raise_before_the_device(bad):
    from dmcf_amd import ops
    from dmcf_amd.utils.tools import losses
    forms = [bad] + ([torch.tensor(bad, dtype=torch.int64)] if all(isinstance(v, int) for v in bad) else [])
    good = [0, 1, 4]
    for rs in forms:
        for kw in (dict(points_row_splits=rs, queries_row_splits=good), dict(points_row_splits=good, queries_row_splits=rs)):
            with pytest.raises(ValueError):
                ops.window_sum(P4, P4.clone(), 0.1, "poly6", **kw)
        for kw in (dict(out_row_splits=rs, in_row_splits=good), dict(out_row_splits=good, in_row_splits=rs)):
            with pytest.raises(ValueError):
                losses.compute_density(P4, P4.clone(), 0.1, win=_poly6(), **kw)
        with pytest.raises(ValueError):
            losses.compute_density(P4, None, 0.1, win=_poly6(), out_row_splits=rs)
        for kw in (dict(row_splits=rs, in_row_splits=good), dict(row_splits=good, in_row_splits=rs)):
            with pytest.raises(ValueError):
                losses.density_loss(P4, P4, P4.clone(), P4.clone(), 0.1, win=_poly6(), **kw)
        with pytest.raises(ValueError):
            losses.density_loss(P4, P4, None, None, 0.1, win=_poly6(), row_splits=rs)


def test_row_splits_types_and_options(monkeypatch):
    from dmcf_amd import ops, _lib
    from dmcf_amd.utils.tools import losses
    i32 = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.window_sum(P4, P4.clone(), 0.1, "poly6", points_row_splits=i32, queries_row_splits=[0, 4])
    with pytest.raises(TypeError):
        losses.compute_density(P4, None, 0.1, win=_poly6(), out_row_splits=i32)
    with pytest.raises(TypeError):
        losses.density_loss(P4, P4, None, None, 0.1, win=_poly6(), row_splits=i32)
    with pytest.raises(ValueError, match="equal lengths"):
        ops.window_sum(P4, Q3, 0.1, "poly6", points_row_splits=[0, 1, 4], queries_row_splits=[0, 3])
    with pytest.raises(ValueError, match="differ"):
        ops.window_sum(P4, P4, 0.1, "poly6", points_row_splits=[0, 1, 4], queries_row_splits=[0, 2, 4])
    with pytest.raises(NotImplementedError, match="window"):
        ops.window_sum(P4, Q3, 0.1, "no such window", points_row_splits=[0, 4], queries_row_splits=[0, 3])
    # an item without rows: the maximum of nothing
    with pytest.raises(ValueError, match="no rows"):
        losses.density_loss(P4, P4, None, None, 0.1, win=_poly6(), row_splits=[0, 1, 1, 4], use_max=True)
    with pytest.raises(ValueError, match="no rows"):
        losses.density_loss(P4, P4, P4.clone(), P4.clone(), 0.1, win=_poly6(), row_splits=[0, 4, 4], in_row_splits=[0, 2, 4])
    # well-formed: on to the device check, as the un-batched call
    with pytest.raises(_lib.DmcfError):
        ops.window_sum(P4, Q3, 0.1, "poly6", points_row_splits=[0, 1, 4], queries_row_splits=[0, 1, 3])
    with pytest.raises(_lib.DmcfError):
        losses.compute_density(Q3, P4, 0.1, win=_poly6(), out_row_splits=[0, 1, 3], in_row_splits=ops.RowSplits([0, 1, 4], None))
    with pytest.raises(_lib.DmcfError):
        losses.density_loss(P4, P4, None, None, 0.1, win=_poly6(), row_splits=[0, 1, 4])
    # the open3d walk emulations know nothing of items
    for name in ("open3d", "open3d_corners"):
        monkeypatch.setenv("DMCF_FRS_SET", name)
        with pytest.raises(NotImplementedError, match="open3d"):
            ops.window_sum(P4, Q3, 0.1, "poly6", points_row_splits=[0, 4], queries_row_splits=[0, 3])
        with pytest.raises(NotImplementedError, match="open3d"):
            losses.compute_density(Q3, P4, 0.1, win=_poly6(), out_row_splits=[0, 3], in_row_splits=[0, 4])
        with pytest.raises(NotImplementedError, match="open3d"):
            losses.density_loss(P4, P4, None, None, 0.1, win=_poly6(), row_splits=[0, 4])


class _NoModel:
    def requires_grad_(self, on):
        return self


class _NoOptimizer:
    def zero_grad(self):
        pass

    def step(self):
        pass


def test_warm_up_batched_defaults_to_off(tmp_path, monkeypatch):
    """A pipeline built without the key takes the per-sample warm-up -- with ``train_batched`` alone too."""
    from dmcf_amd.pipelines.simulator import Simulator
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    taken = []
    for kwargs, want in ((dict(), "looped"), (dict(train_batched=True), "looped"), (dict(warm_up_batched=False), "looped"),
                         (dict(warm_up_batched=True), "batched"), (dict(train_batched=True, warm_up_batched=True), "batched")):
        sim = Simulator(_NoModel(), device="cuda", main_log_dir=str(tmp_path), **kwargs)
        assert bool(sim.cfg.get("warm_up_batched", False)) is (want == "batched")
        sim.device = torch.device("cpu")  # (everything below is a stub: nothing reaches a device)
        sim.optimizer = _NoOptimizer()
        sim.warm_up = lambda *a: taken.append("looped") or ([], [], [0])
        sim.warm_up_batched = lambda *a: taken.append("batched") or ([], [], [0])
        sim.window_loss = lambda *a: torch.ones(2, requires_grad=True) * 2
        loss, pre = sim.train_step(dict(pos=[None]), [1.0], max_dens_err=0.1)
        assert taken[-1] == want and pre == [0] and loss.tolist() == [2.0, 2.0]


# ---- the exit bookkeeping -------------------------------------------------------------------------------------------------------
def test_warm_up_exits_restates_the_loop():
    """WarmUpExits against the loop's own lines, on error sequences that take every branch."""
    from dmcf_amd.pipelines.simulator import WarmUpExits

    def loop(pre, errs, dens, max_err, max_dens_err):  # simulator.py's warm_up, its decisions only
        p, prev_err, prev_dens_err, taken = 0, 0.0, 0.0, []
        for p in range(pre):
            if max_err is not None:
                if p > 0 and errs[p] > prev_err and errs[p] > max_err:
                    break
                prev_err = errs[p]
            if max_dens_err is not None:
                if p > 0 and dens[p] > prev_dens_err and dens[p] > max_dens_err:
                    break
                prev_dens_err = dens[p]
            taken.append(p)
        return p, taken

    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(300):
        pre = int(rng.integers(0, 7))
        errs, dens = rng.uniform(0, 2, size=pre).tolist(), rng.uniform(0, 2, size=pre).tolist()
        max_err = [None, 0.5, 1.0][int(rng.integers(0, 3))]
        max_dens_err = [None, 0.5, 1.0][int(rng.integers(0, 3))]
        want_p, want_taken = loop(pre, errs, dens, max_err, max_dens_err)
        ex = WarmUpExits([pre], max_err, max_dens_err)
        taken = []
        for p in range(pre):
            if ex.active(p) != [0]:
                break
            if ex.accept(p, 0, errs[p], dens[p]):
                taken.append(p)
        assert ex.pres() == [want_p] and taken == want_taken
        seen.add((pre == 0, want_p < pre - 1))
    assert seen == {(True, False), (False, False), (False, True)}


class _Drift:
    """A model on CPU tensors whose step moves every particle of a sample by that sample's own constant drift (the drift
    rides in the velocity).  ``__call__`` is the per-sample step, ``step_batched`` the same for a list of items."""

    def __init__(self):
        self.batches, self.calls = [], 0

    def __call__(self, inputs, training=False):
        self.calls += 1
        return inputs[0] + inputs[1], inputs[1]

    def step_batched(self, items, training=False):
        self.batches.append(len(items))
        rs = [0]
        for it in items:
            rs.append(rs[-1] + it[0].shape[0])
        pos, vel = torch.cat([it[0] for it in items]), torch.cat([it[1] for it in items])
        return pos + vel, vel, rs


PRE = [0, 1, 4, 6, 6]


def _drift_data():
    """Five samples, pre = [0, 1, 4, 6, 6]; frame p of a sample is p0 + min(p, last) * drift.  The state after p + 1 steps,
    p0 + (p + 1) * drift, is compared with frame p: while the frames follow the drift the error is the constant 2 d (never
    above its predecessor: no exit), and from the first frame that stays behind it grows.  Sample 2 (d = 1/8) stays at frame
    1: errors 1/4, 1/4, 1/2 -- it leaves at p = 2 under max_err = 3/8; sample 3 (d = 1/4) stays at frame 3: errors 1/2 four
    times, then 1 -- it leaves at p = 4; the others follow to the end.  Every number is exact in float32."""
    sizes = [3, 2, 4, 5, 3]
    drift = [0.5, 0.0625, 0.125, 0.25, 0.0625]
    last = {2: 1, 3: 3}
    rng = np.random.default_rng(11)
    data = dict(pos=[], vel=[], grav=[], box=[], box_normals=[], pre=PRE)
    for bi, (n, d) in enumerate(zip(sizes, drift)):
        p0 = (rng.integers(0, 64, size=(n, 3)) / 8.0).astype(np.float32)
        step = np.array([d, 0.0, d], dtype=np.float32)
        data["pos"].append(np.stack([p0 + np.float32(min(p, last.get(bi, 99))) * step for p in range(8)]))
        data["vel"].append(np.broadcast_to(step, (8, n, 3)).astype(np.float32).copy())
        data["grav"].append([None] * 8)
        data["box"].append(np.zeros((8, 1, 3), dtype=np.float32))
        data["box_normals"].append(np.zeros((8, 1, 3), dtype=np.float32))
    return data


MAX_ERR = 0.375


def _both_warm_ups(tmp_path):
    from dmcf_amd.pipelines.simulator import Simulator
    data = _drift_data()
    model = _Drift()
    sim = Simulator(model, device="cuda", main_log_dir=str(tmp_path))
    sim.device = torch.device("cpu")  # (the model is a stub on CPU tensors: nothing reaches a device)
    want = sim.warm_up(data, max_err=MAX_ERR)
    assert model.batches == [] and model.calls == sum(min(k, at + 1) for k, at in zip(PRE, want[2]))
    got = sim.warm_up_batched(data, max_err=MAX_ERR)
    return want, got, model.batches


def test_warm_up_batched_on_the_host(tmp_path):
    """max_err only, on CPU tensors: the batched warm-up returns what the per-sample loop returns, bit for bit."""
    (want_pos, want_vel, want_pre), (got_pos, got_vel, got_pre), _ = _both_warm_ups(tmp_path)
    # one sample leaves at p = 2, one at p = 4, one never; pre == 0 records 0 with frame 0's state; a whole run records pre - 1
    assert want_pre == [0, 0, 2, 4, 5]
    assert got_pre == want_pre
    assert len(got_pos) == len(got_vel) == 5
    for a, b in zip(want_pos + want_vel, got_pos + got_vel):
        assert a.shape == b.shape and torch.equal(a, b)


def test_warm_up_batched_batches_follow_the_exits(tmp_path):
    """Items that have left or finished are not in the next iteration's batch."""
    batches = _both_warm_ups(tmp_path)[2]
    # p = 0: samples 1 - 4; p = 1, 2: 2, 3, 4 (2 leaves at p = 2); p = 3, 4: 3, 4 (3 leaves at p = 4); p = 5: 4
    assert batches == [4, 3, 3, 2, 2, 1]


def test_warm_up_batched_refuses_a_model_without_a_batched_step(tmp_path):
    from dmcf_amd import models
    from dmcf_amd.pipelines.simulator import Simulator
    from tools import configs
    data = _drift_data()
    sim = Simulator(_NoModel(), device="cuda", main_log_dir=str(tmp_path))
    sim.device = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="step_batched"):
        sim.warm_up_batched(data, max_err=0.25)
    cfg = configs.CCONV2D
    sim.model = getattr(models, cfg["name"])(**cfg)
    with pytest.raises(NotImplementedError, match=cfg["name"]):
        sim.warm_up_batched(data, max_err=0.25)
