"""The batched validation on the GPU: dmcf_nn_distance_ragged against the dense call on every item alone (bit for bit),
chamfer_distance with row splits, Simulator.run_rollout_batched against run_rollout, and run_valid with the pipeline key
``valid_batched`` against the per-scene loop.

Shapes.  The kernel's batch has item sizes (n, m) = (1, 1), (63, 65), (64, 64), (65, 1), (0, 0), (257, 300), (600, 700) and
(125, 125): both edges of a 64-row tile, more than one 256-point LDS tile of the other set in both directions, an item with
both sets empty, and a 5 x 5 x 5 lattice against itself shifted by half a spacing, where every row has exact ties (spacing 1/4,
shift 1/8: every distance is exact in float32).  The pipeline tests use the scenes of tests/batched_scene.py and the scaled
WaterRamps-pattern SymNet of tests/test_gpu_step_batched.py, whose 1e-5 bar for one step (one float32 ulp of a position at
these speeds) is taken over as it is."""
import tempfile
import types

import numpy as np
import pytest

import batched_scene as scene
import metrics_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(1, 1), (63, 65), (64, 64), (65, 1), (0, 0), (257, 300), (600, 700), (125, 125)]
LATTICE = 7


def _splits(counts):
    rs = [0]
    for c in counts:
        rs.append(rs[-1] + c)
    return rs


def _batch(seed=0):
    rng = np.random.default_rng(seed)
    a = [rng.uniform(-1, 1, size=(n, 3)).astype(np.float32) for n, _ in SIZES]
    b = [rng.uniform(-1, 1, size=(m, 3)).astype(np.float32) for _, m in SIZES]
    g = np.arange(5, dtype=np.float32) * 0.25
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    a[LATTICE], b[LATTICE] = lattice + np.float32(0.125), lattice
    return a, b


@pytest.fixture(scope="module")
def ragged():
    """The batch, the ragged call's four outputs and the dense call on every item alone (the parent's code), computed once."""
    from dmcf_amd import ops
    a, b = _batch()
    rs1, rs2 = _splits([n for n, _ in SIZES]), _splits([m for _, m in SIZES])
    A, B = torch.from_numpy(np.concatenate(a)).to(DEV), torch.from_numpy(np.concatenate(b)).to(DEV)
    got = ops.nn_distance(A, B, rs1, rs2)
    per_item = [ops.nn_distance(A[rs1[k]:rs1[k + 1]], B[rs2[k]:rs2[k + 1]]) if n else None for k, (n, _) in enumerate(SIZES)]
    return dict(a=a, b=b, A=A, B=B, rs1=rs1, rs2=rs2, got=got, per_item=per_item)


def _assert_items_equal(got, per_item, rs1, rs2):
    d1, i1, d2, i2 = got
    for k, want in enumerate(per_item):
        if want is None:
            continue
        s1, s2 = slice(rs1[k], rs1[k + 1]), slice(rs2[k], rs2[k + 1])
        if d1 is not None:
            assert torch.equal(d1[s1], want[0]), k
            assert torch.equal(i1[s1] - rs2[k], want[1]), k
        if d2 is not None:
            assert torch.equal(d2[s2], want[2]), k
            assert torch.equal(i2[s2] - rs1[k], want[3]), k


def test_every_item_has_the_dense_calls_bits(ragged):
    d1, i1, d2, i2 = ragged["got"]
    n, m = ragged["rs1"][-1], ragged["rs2"][-1]
    assert d1.shape == (n,) and i1.shape == (n,) and d2.shape == (m,) and i2.shape == (m,)
    assert d1.dtype == d2.dtype == torch.float32 and i1.dtype == i2.dtype == torch.int32
    _assert_items_equal(ragged["got"], ragged["per_item"], ragged["rs1"], ragged["rs2"])
    # the lattice item: a shifted point is equally far from the 8 corners of its cell (3/64, exact); the lowest index wins
    k = LATTICE
    want1 = ragged["per_item"][k]
    assert torch.all(want1[0] == 3 * 0.125 ** 2)
    corner = torch.arange(125, device=DEV).view(5, 5, 5)
    assert torch.equal(want1[1].view(5, 5, 5)[:4, :4, :4].long(), corner[:4, :4, :4])


def test_one_direction_forms(ragged):
    from dmcf_amd import ops
    A, B, rs1, rs2 = ragged["A"], ragged["B"], ragged["rs1"], ragged["rs2"]
    only1 = ops.nn_distance_ragged(A, B, rs1, rs2, want2=False)
    only2 = ops.nn_distance_ragged(A, B, rs1, rs2, want1=False)
    assert only1[2] is None and only1[3] is None and only2[0] is None and only2[1] is None
    for k in (0, 1):
        assert torch.equal(only1[k], ragged["got"][k]) and torch.equal(only2[k + 2], ragged["got"][k + 2])
    # the splits in their other forms: device tensors, RowSplits
    dev_rs = [torch.tensor(rs, dtype=torch.int64, device=DEV) for rs in (rs1, rs2)]
    for s1, s2 in ((dev_rs[0], dev_rs[1]), (ops.RowSplits(rs1, dev_rs[0]), tuple(rs2))):
        for x, y in zip(ops.nn_distance(A, B, s1, s2), ragged["got"]):
            assert torch.equal(x, y)


def test_indices_against_float64(ragged):
    """tests/metrics_ref.nn_distance in float64 on the items without ties: the same index wherever float32 can tell the
    nearest from the second nearest (a gap above 1e-5 relative; float32 squared distances carry ~3 ulp = 2e-7), and a
    float64 distance to the chosen point within 1e-5 relative of the smallest everywhere."""
    d1, i1, d2, i2 = (x.cpu().numpy() for x in ragged["got"])
    rs1, rs2 = ragged["rs1"], ragged["rs2"]
    checked = 0
    for k, (n, m) in enumerate(SIZES):
        if n == 0 or k == LATTICE:
            continue
        a, b = ragged["a"][k], ragged["b"][k]
        ref = metrics_ref.nn_distance(a[None], b[None])
        for q, p, dist, idx, off, rd, ri in ((a, b, d1[rs1[k]:rs1[k + 1]], i1[rs1[k]:rs1[k + 1]], rs2[k], ref[0][0], ref[1][0]),
                                             (b, a, d2[rs2[k]:rs2[k + 1]], i2[rs2[k]:rs2[k + 1]], rs1[k], ref[2][0], ref[3][0])):
            local = idx - off
            assert local.min() >= 0 and local.max() < len(p)
            sq = metrics_ref.sqdist(q, p)
            chosen = sq[np.arange(len(q)), local]
            assert np.all(chosen <= rd * (1 + 1e-5) + 1e-12)
            assert np.allclose(dist, rd, rtol=1e-5, atol=1e-12)
            second = np.partition(sq, 1, axis=1)[:, 1] if len(p) > 1 else np.full(len(q), np.inf)
            clear = second > rd * (1 + 1e-5) + 1e-12
            assert np.array_equal(local[clear], ri[clear])
            checked += int(clear.sum())
    assert checked > 1500  # (nearly every row of the untied items)


def test_items_do_not_see_each_other(ragged):
    from dmcf_amd import ops
    rs1, rs2 = ragged["rs1"], ragged["rs2"]
    A, B = ragged["A"].clone(), ragged["B"].clone()
    A[rs1[5]:rs1[6]] += 0.37  # item 5 moves ...
    B[rs2[5]:rs2[6]] -= 0.21
    moved = ops.nn_distance(A, B, rs1, rs2)
    for x, y, rs in zip(moved, ragged["got"], (rs1, rs1, rs2, rs2)):
        keep = torch.ones(x.shape[0], dtype=torch.bool, device=DEV)
        keep[rs[5]:rs[6]] = False
        assert torch.equal(x[keep], y[keep])  # ... and every other item's four outputs stay bit-identical
    assert not torch.equal(moved[0][rs1[5]:rs1[6]], ragged["got"][0][rs1[5]:rs1[6]])
    # two items at identical coordinates give identical results
    a, b = ragged["a"], ragged["b"]
    twice_a, twice_b = [a[5], a[1], a[5]], [b[5], b[1], b[5]]
    s1, s2 = _splits([len(x) for x in twice_a]), _splits([len(x) for x in twice_b])
    d1, i1, d2, i2 = ops.nn_distance(torch.from_numpy(np.concatenate(twice_a)).to(DEV),
                                     torch.from_numpy(np.concatenate(twice_b)).to(DEV), s1, s2)
    assert torch.equal(d1[s1[0]:s1[1]], d1[s1[2]:s1[3]]) and torch.equal(d2[s2[0]:s2[1]], d2[s2[2]:s2[3]])
    assert torch.equal(i1[s1[0]:s1[1]] - s2[0], i1[s1[2]:s1[3]] - s2[2])
    assert torch.equal(i2[s2[0]:s2[1]] - s1[0], i2[s2[2]:s2[3]] - s1[2])
    assert torch.equal(d1[s1[0]:s1[1]], ragged["per_item"][5][0])


def test_chamfer_distance_with_splits(ragged):
    from dmcf_amd.utils.evaluation_helper import chamfer_distance
    rs1, rs2 = ragged["rs1"], ragged["rs2"]
    # (pred = the second set, gt = the first: for each point of gt the distance to its nearest point of pred)
    got = chamfer_distance(ragged["B"], ragged["A"], pred_row_splits=rs2, gt_row_splits=rs1)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (rs1[-1],)
    from_numpy = chamfer_distance(np.concatenate(ragged["b"]), np.concatenate(ragged["a"]), pred_row_splits=rs2, gt_row_splits=rs1)
    assert np.array_equal(got, from_numpy)
    for k, (n, _) in enumerate(SIZES):
        if n:
            want = chamfer_distance(ragged["B"][rs2[k]:rs2[k + 1]], ragged["A"][rs1[k]:rs1[k + 1]])
            assert np.array_equal(got[rs1[k]:rs1[k + 1]], want), k


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
def _rel(a, b):  # as tests/test_gpu_step_batched.py defines it
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _scenes(which, frames):
    """Scenes of tests/batched_scene.py as get_rollout returns them: [T, N, 3] arrays; the targets drift with the velocity."""
    from test_gpu_step_batched import _items
    items = _items("waterramps")
    data = []
    for b in which:
        p0, v0, acc, _, box, nrm = (x.cpu().numpy() if x is not None else None for x in items[b])
        pos = np.stack([p0 + k * 0.0025 * v0 + np.float32(1e-3 * k) for k in range(frames)]).astype(np.float32)
        rep = lambda x: np.broadcast_to(x, (frames,) + x.shape).copy()  # noqa: E731
        data.append(dict(pos=pos, vel=rep(v0), grav=rep(acc), box=rep(box), box_normals=rep(nrm)))
    return data


@pytest.fixture(scope="module")
def model():
    from test_gpu_step_batched import _model
    return _model("waterramps")


def test_run_rollout_batched_against_run_rollout(model):
    from dmcf_amd.pipelines.simulator import Simulator
    data = _scenes((0, 1, 2), 2)
    sim = Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp())
    want = sim.run_rollout(data, 2)
    got = sim.run_rollout_batched(data, 2)
    assert len(sim.timing) == 1
    for i, n in enumerate(scene.COUNTS):
        assert len(got[i]) == len(want[i]) == 2
        assert torch.equal(got[i][0][0], want[i][0][0]) and torch.equal(got[i][0][1], want[i][0][1])
        assert got[i][1][0].shape == got[i][1][1].shape == (n, 3)
        ep = _rel(got[i][1][0].cpu().numpy(), want[i][1][0].cpu().numpy())
        ev = _rel(got[i][1][1].cpu().numpy(), want[i][1][1].cpu().numpy())
        print(f"scene {i}: frame 1 pos rel {ep:.2e}, vel rel {ev:.2e}")
        assert ep <= 1e-5 and ev <= 1e-5, (i, ep, ev)
    # four frames: the structure only (differences compound through (pos' - pos) / dt; nobody has measured how fast)
    got = sim.run_rollout_batched(data, 4)
    assert len(sim.timing) == 3
    for i, n in enumerate(scene.COUNTS):
        assert len(got[i]) == 4
        for t in range(4):
            pos, vel, acc, feats, box, bfeats = got[i][t]
            assert pos.shape == vel.shape == (n, 3) and torch.isfinite(pos).all() and torch.isfinite(vel).all()
            assert feats is None and acc is got[i][0][2] and box is got[i][0][4] and bfeats is got[i][0][5]


EXACT = ("mse_val", "chamfer_val", "chamfer_val_2", "emd", "vel_diff_val", "vel_diff_val_2")
KEYS = set(EXACT) | {"dens_val", "max_dens_val", "mse_single_val", "loss"}


class _Counting:
    """The library with a counter on every entry point called (the pattern of tests/test_gpu_step_batched.py)."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dmcf_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.fixture(scope="module")
def valid_runs(model):
    """run_valid on a two-scene, three-frame in-memory split: looped (the parent's path), with ``valid_batched`` on the looped
    rollout's results (the metrics stage alone), and with ``valid_batched`` end to end under the counting library."""
    from dmcf_amd import _lib, datasets
    from dmcf_amd.pipelines.simulator import Simulator
    data = _scenes((0, 2), 3)
    mp = pytest.MonkeyPatch()
    res = dict(data=data)
    try:
        mp.setattr(datasets, "get_rollout", lambda *a, **k: data)

        def sim(**kw):
            return Simulator(model, dataset=types.SimpleNamespace(valid=None), device="cuda", main_log_dir=tempfile.mkdtemp(),
                             split="valid", **kw)
        looped = sim()
        rollout, kept = looped.run_rollout, []
        looped.run_rollout = lambda *a: kept.append(rollout(*a)) or kept[-1]
        counting = _Counting(_lib.lib())
        mp.setattr(_lib, "lib", lambda: counting)
        res["looped"] = dict(looped.run_valid(epoch=0))
        res["looped_calls"] = dict(counting.calls)
        staged = sim(valid_batched=True)
        staged.run_rollout_batched = lambda *a: kept[0]
        res["staged"] = dict(staged.run_valid(epoch=0))
        counting.calls.clear()
        whole = sim(valid_batched=True)
        res["whole"] = dict(whole.run_valid(epoch=0))
        res["whole_calls"] = dict(counting.calls)
        assert whole.valid_loss == res["whole"]
    finally:
        mp.undo()
    return res


def test_metrics_stage_against_the_loop(valid_runs):
    want, got = valid_runs["looped"], valid_runs["staged"]
    print("looped ", want)
    print("batched", got)
    assert list(got) == list(want) and set(got) == KEYS  # (the same keys in the same order: the log line is the loop's)
    for k in EXACT:
        assert got[k] == want[k], k
    for k in ("dens_val", "max_dens_val"):
        assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]), (k, got[k], want[k])
    biggest = max(float(np.abs(d["pos"]).max()) for d in valid_runs["data"])
    assert abs(got["mse_single_val"] - want["mse_single_val"]) <= 1e-5 * biggest
    assert got["loss"] == sum(v for k, v in got.items() if k != "loss")


def test_run_valid_batched_end_to_end(valid_runs):
    want, got, calls = valid_runs["looped"], valid_runs["whole"], valid_runs["whole_calls"]
    print("batched end to end", got)
    assert list(got) == list(want)
    assert all(np.isfinite(v) for v in got.values())
    assert got["loss"] == sum(v for k, v in got.items() if k != "loss")
    # two evaluated frames: one ragged call each serves chamfer_val and chamfer_val_2; the dense entry point is not called
    assert calls.get("dmcf_nn_distance_ragged", 0) == 2
    assert calls.get("dmcf_nn_distance", 0) == 0
    assert valid_runs["looped_calls"].get("dmcf_nn_distance", 0) == 2 * 2 * 2  # (scenes x frames x directions)
    assert valid_runs["looped_calls"].get("dmcf_nn_distance_ragged", 0) == 0
