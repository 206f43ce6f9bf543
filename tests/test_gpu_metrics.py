"""The validation metrics on the GPU (dmcf_amd/csrc/metrics.hip): nn_distance against a float64 brute force; approx_match,
match_cost and the fused emd against the float64 restatement tests/metrics_ref.py; padding, 2-D sets and bitwise
repeatability; Simulator.run_valid end to end on the canyon fixture with every metric recomputed independently (cKDTree in
float64, the restatement, compute_density), also through run_pipeline --split valid and run_test's test_compute_metric."""
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import metrics_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24
WORST = {}  # largest err / bar seen per check (printed at the end of the module)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    yield torch.device("cuda:0")
    print("\nworst err/bar:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ----------------------------------------------------------------------------------------------------------------------
# nn_distance
# ----------------------------------------------------------------------------------------------------------------------
def _sq(a, b):
    """float64 [n, m] squared distances, one coordinate at a time (no [n, m, 3] temporary)."""
    a, b = R._pad3(a).astype(np.float64), R._pad3(b).astype(np.float64)
    d = np.zeros((len(a), len(b)))
    for k in range(3):
        d += (a[:, k, None] - b[None, :, k]) ** 2
    return d


def _check_direction(q, p, dist, idx, key):
    d = _sq(q, p)
    dmin = d.min(1)
    bar = 8 * U * dmin + 1e-37
    err = np.abs(dist.astype(np.float64) - dmin)
    _note(key, (err / bar).max())
    assert (err <= bar).all(), (err / bar).max()
    # indices: equal wherever the runner-up is not within rounding; exact duplicates go to the lowest index
    near = d <= (dmin * (1 + 32 * U) + 1e-37)[:, None]
    ambiguous = near.sum(1) > 1
    first = d.argmin(1)
    assert np.array_equal(idx[~ambiguous], first[~ambiguous])
    for i in np.nonzero(ambiguous)[0]:
        cand = np.nonzero(near[i])[0]
        assert idx[i] in cand
        pts = R._pad3(p)[cand]
        if (pts == pts[0]).all():  # all tied candidates are the same point: the lowest index wins
            assert idx[i] == cand[0]


def _run_nn(a, b, dev, key):
    d1, i1, d2, i2 = (x.cpu().numpy() for x in __import__("dmcf_amd.ops", fromlist=["ops"]).nn_distance(_t(a, dev), _t(b, dev)))
    for k in range(a.shape[0]):
        _check_direction(a[k], b[k], d1[k], i1[k], key)
        _check_direction(b[k], a[k], d2[k], i2[k], key)
    return d1, i1, d2, i2


SIZES = [1, 63, 64, 65, 1000, 4097]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", SIZES)
def test_nn_distance_brute_force(dev, n, m):
    rng = np.random.default_rng(n * 10007 + m)
    a = rng.uniform(-1, 1, (1, n, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, (1, m, 3)).astype(np.float32)
    _run_nn(a, b, dev, "nn_distance")


@pytest.mark.parametrize("n,m", [(65, 1000), (4097, 63), (1, 64), (1000, 1000)])
def test_nn_distance_batched_2d_and_duplicates(dev, n, m):
    from dmcf_amd import ops
    rng = np.random.default_rng(n + 3 * m)
    a = rng.uniform(0, 1, (3, n, 3)).astype(np.float32)
    b = rng.uniform(0, 1, (3, m, 3)).astype(np.float32)
    # duplicated points: copies of earlier points (and of query points) at higher indices
    b[:, m // 2:] = b[:, :m - m // 2]
    if m > 3:
        b[1, 1] = a[1, 0]
        b[1, 3] = a[1, 0]
    out = _run_nn(a, b, dev, "nn_distance")
    if m > 3:
        assert out[1][1, 0] == 1 and out[0][1, 0] == 0.0
    # 2-D sets: z = 0, the same bits as the zero-padded 3-D call
    a2, b2 = a[:, :, :2].copy(), b[:, :, :2].copy()
    got = ops.nn_distance(_t(a2, dev), _t(b2, dev))
    pad = ops.nn_distance(_t(R._pad3(a2), dev), _t(R._pad3(b2), dev))
    for x, y in zip(got, pad):
        assert torch.equal(x, y)
    _run_nn(a2, b2, dev, "nn_distance_2d")
    # unbatched [n, 3]: the first item of the batched call
    single = ops.nn_distance(_t(a[0], dev), _t(b[0], dev))
    for x, y in zip(single, out):
        np.testing.assert_array_equal(x.cpu().numpy(), y[0])


# ----------------------------------------------------------------------------------------------------------------------
# approx_match / match_cost / emd
# ----------------------------------------------------------------------------------------------------------------------
MATCH_CASES = [(1, 1, 1.0), (7, 3, 1.0), (3, 7, 1.0), (63, 65, 1.0), (64, 64, 0.2), (1000, 1999, 1.0), (1999, 1000, 0.3),
               (4097, 1000, 1.0), (500, 500, 0.05)]


@pytest.mark.parametrize("n,m,scale", MATCH_CASES)
def test_approx_match_against_restatement(dev, n, m, scale):
    """Element-wise bar |err| <= 2^-5 (|ref| + max|ref| / 64): the same expression evaluated in float32 (metrics_ref with
    dtype=float32) stays below 2^-8 of it; the iteration subtracts O(max) terms (remainR - s, remainL - sum w), so entries
    near zero carry errors of the size of the largest ones."""
    from dmcf_amd import ops
    rng = np.random.default_rng(n * 31 + m)
    a = rng.uniform(0, scale, (1, n, 3)).astype(np.float32)
    b = rng.uniform(0, scale, (1, m, 3)).astype(np.float32)
    A, B = _t(a, dev), _t(b, dev)
    match = ops.approx_match(A, B)
    got = match.cpu().numpy().astype(np.float64)
    ref, sc = R.match_abs_scale(a, b)
    ratio = np.abs(got - ref) / (2.0 ** -5 * sc)
    _note("approx_match", ratio.max())
    assert ratio.max() <= 1.0, ratio.max()
    assert (got >= 0).all()
    ml, mr = R.multipliers(n, m)
    assert (got.sum(1) <= ml * (1 + 1e-4)).all() and (got.sum(2) <= mr * (1 + 1e-4)).all()
    # match_cost of the GPU match against float64 on the same match, and against the float64 plan's cost
    cost = ops.match_cost(A, B, match).cpu().numpy()
    want_same = R.match_cost(a, b, got)
    assert np.abs(cost - want_same).max() <= 1e-5 * want_same.max() + 1e-30
    want = R.match_cost(a, b, ref)
    _note("match_cost", (np.abs(cost - want) / (1e-4 * want + 1e-30)).max())
    assert np.abs(cost - want).max() <= 1e-4 * want.max() + 1e-30
    # the fused EMD: no match formed, the same cost within a bar
    e = ops.emd(A, B).cpu().numpy()
    _note("emd_vs_match_cost", (np.abs(e - cost) / (1e-5 * cost + 1e-30)).max())
    assert np.abs(e - cost).max() <= 1e-5 * cost.max() + 1e-30
    assert np.abs(e - want).max() <= 1e-4 * want.max() + 1e-30


def test_approx_match_padded_counts_and_repeatable(dev):
    """Per-batch counts: the padded batch gives exactly the unpadded items' bits, with zeros in the padding; the padding's
    coordinates play no part.  Two identical calls give identical bits."""
    from dmcf_amd import ops
    rng = np.random.default_rng(11)
    counts_n, counts_m = [700, 1999, 5], [1000, 640, 3]
    N, M = 2000, 1024
    a = rng.uniform(50, 60, (3, N, 3)).astype(np.float32)  # padding far away
    b = rng.uniform(-60, -50, (3, M, 3)).astype(np.float32)
    for i in range(3):
        a[i, :counts_n[i]] = rng.uniform(0, 1, (counts_n[i], 3))
        b[i, :counts_m[i]] = rng.uniform(0, 1, (counts_m[i], 3))
    A, B = _t(a, dev), _t(b, dev)
    match = ops.approx_match(A, B, counts_n, torch.tensor(counts_m))
    assert torch.equal(match, ops.approx_match(A, B, counts_n, counts_m))
    e = ops.emd(A, B, counts_n, counts_m)
    assert torch.equal(e, ops.emd(A, B, counts_n, counts_m))
    for i in range(3):
        one = ops.approx_match(A[i:i + 1, :counts_n[i]], B[i:i + 1, :counts_m[i]])[0]
        mi = match[i]
        assert torch.equal(mi[:counts_m[i], :counts_n[i]], one)
        assert not mi[counts_m[i]:].any() and not mi[:, counts_n[i]:].any()
        assert torch.equal(e[i], ops.emd(A[i:i + 1, :counts_n[i]], B[i:i + 1, :counts_m[i]])[0])
    # zero counts: an empty item costs 0
    z = ops.emd(A[:1], B[:1], [0], [5])
    assert z.item() == 0.0
    # nn_distance is repeatable too
    r1 = ops.nn_distance(A, B)
    r2 = ops.nn_distance(A, B)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))


def test_emd_2d_and_emd_loss(dev):
    from dmcf_amd import ops
    from dmcf_amd.utils.tools.losses import emd_loss
    rng = np.random.default_rng(2)
    a = rng.uniform(0, 1, (2, 300, 2)).astype(np.float32)
    b = rng.uniform(0, 1, (2, 200, 2)).astype(np.float32)
    A, B = _t(a, dev), _t(b, dev)
    assert torch.equal(ops.emd(A, B), ops.emd(_t(R._pad3(a), dev), _t(R._pad3(b), dev)))
    want = R.match_cost(a, b, R.approx_match(a, b))
    got = emd_loss(A, B).cpu().numpy()
    np.testing.assert_allclose(got, want / 300, rtol=1e-4)
    got_c = emd_loss(A, B, n=[300, 100], m=[200, 150]).cpu().numpy()
    want_c = R.match_cost(a[1:, :100], b[1:, :150], R.approx_match(a[1:, :100], b[1:, :150]))[0] / 150
    np.testing.assert_allclose(got_c[1], want_c, rtol=1e-4)


def test_approx_match_refuses_what_does_not_fit(dev):
    from dmcf_amd import ops
    a = torch.zeros((1, 400000, 3), device=dev)  # a 640 GB match
    with pytest.raises(MemoryError, match="ops.emd"):
        ops.approx_match(a, a)


# ----------------------------------------------------------------------------------------------------------------------
# run_valid end to end
# ----------------------------------------------------------------------------------------------------------------------
REF_KEYS = {"mse_val", "chamfer_val", "dens_val", "max_dens_val", "chamfer_val_2", "emd", "vel_diff_val", "vel_diff_val_2",
            "mse_single_val", "loss"}


def _yaml(tmp_path, extra_pipeline=None):
    import yaml
    tmp_path.mkdir(parents=True, exist_ok=True)
    from tools import configs
    valid = dict(stride=1, time_end=3)
    cfg = dict(dataset=dict(name="CConvData3D"),
               model=dict(configs.LIQUID3D, ckpt_path=None),
               pipeline=dict(name="Simulator", version="v0", main_log_dir=str(tmp_path / "logs"), output_dir=str(tmp_path / "out"),
                             data_generator=dict(scale=[1.0, 1.0, 1.0], train=dict(stride=1), valid=valid,
                                                 test=dict(stride=1, time_start=0, time_end=3)), **(extra_pipeline or {})))
    yml = tmp_path / "liquid3d.yml"
    yml.write_text(yaml.safe_dump(cfg))
    return str(yml)


def _weights():
    return dict(np.load(os.path.join(GOLDEN, "liquid3d_weights.npz")))


def _expected(pipe, dev):
    """Every metric of run_valid recomputed from a fresh rollout of the same scene: host float64 (cKDTree, the EMD
    restatement, a per-point histogram loop) where the metric allows, compute_density for the densities."""
    from scipy.spatial import cKDTree
    from test_metrics_abi import _compare_dist_loop
    from dmcf_amd.datasets import get_rollout
    from dmcf_amd.utils.tools.losses import compute_density, get_window_func
    data = get_rollout(pipe.dataset.valid, scale=[1.0, 1.0, 1.0], stride=1, time_end=3)[0]
    results = pipe.run_rollout([data], data["pos"].shape[0])[0]
    box = data["box"][0]
    lo, hi = box.min(0), box.max(0)
    per = []
    for t in range(1, data["pos"].shape[0]):
        tgt, tv = data["pos"][t].astype(np.float64), data["vel"][t]
        pos = np.clip(results[t][0].cpu().numpy(), lo, hi).astype(np.float64)
        vel = results[t][1].cpu().numpy()
        e = {"mse_val": np.linalg.norm(tgt - pos, axis=-1).mean(),
             "chamfer_val": cKDTree(tgt).query(pos)[0].mean(),
             "chamfer_val_2": cKDTree(pos).query(tgt)[0].mean()}
        P, T, Bx = _t(pos, dev), _t(tgt, dev), _t(box, dev)
        dens = lambda o, i, r, w: compute_density(o, i, r, win=w).double().cpu().numpy()  # noqa: E731
        poly6 = get_window_func("poly6")
        # density_loss(gt=target, pred=pos, gt_in=pos + box, pred_in=target + box): the reference's order
        pd, gd = dens(P, torch.cat([T, Bx]), 0.005, poly6), dens(T, torch.cat([P, Bx]), 0.005, poly6)
        e["dens_val"] = np.maximum(pd - gd.max() - 0.01, 0).mean()
        win = get_window_func(pipe.model.window_dens)
        r0 = pipe.model.particle_radii[0]
        pd, gd = dens(T, torch.cat([T, Bx]), r0, win), dens(P, torch.cat([P, Bx]), r0, win)
        e["max_dens_val"] = abs(pd.max() - gd.max()) / gd.max()
        a32, b32 = tgt.astype(np.float32)[None], pos.astype(np.float32)[None]
        e["emd"] = R.match_cost(a32, b32, R.approx_match(a32, b32))[0] / len(tgt)
        e["vel_diff_val"] = _compare_dist_loop(tv, vel)
        e["vel_diff_val_2"] = _compare_dist_loop(vel, tv)
        g = data.get("grav")
        one = pipe.run_inference([[_t(data["pos"][t - 1], dev), _t(data["vel"][t - 1], dev), _t(g[t - 1], dev) if g is not None
                                   else None, None, _t(box, dev), _t(data["box_normals"][0], dev)]])[0][0].cpu().numpy()
        e["mse_single_val"] = np.linalg.norm(data["pos"][t] - one, axis=-1).mean()
        per.append(e)
    out = {k: float(np.mean([e[k] for e in per])) for k in per[0]}
    out["loss"] = sum(out.values())
    return out


TOL = {"mse_val": 1e-5, "chamfer_val": 1e-5, "chamfer_val_2": 1e-5, "dens_val": 1e-4, "max_dens_val": 1e-4, "emd": 1e-4,
       "vel_diff_val": 1e-9, "vel_diff_val_2": 1e-9, "mse_single_val": 1e-6, "loss": 1e-4}


def _check_metrics(got, want):
    assert set(got) == REF_KEYS
    for k in REF_KEYS:
        assert np.isfinite(got[k]), k
        assert abs(got[k] - want[k]) <= TOL[k] * max(abs(want[k]), 1e-3), (k, got[k], want[k])


def test_run_valid_on_canyon(dev, tmp_path):
    from dmcf_amd import run_pipeline
    from dmcf_amd.utils import tf_checkpoint as tc
    args, extra = run_pipeline.parse_args(["-c", _yaml(tmp_path), "--split", "valid", "--dataset_path", GOLDEN])
    pipe = run_pipeline.build(args, extra)
    tc.load_into_model(pipe.model, _weights(), device=dev)
    got = pipe.run_valid()
    assert got is pipe.valid_loss
    want = _expected(pipe, dev)
    _check_metrics(got, want)
    logs = glob.glob(os.path.join(pipe.cfg.logs_dir, "log_valid_*.txt"))
    assert len(logs) == 1
    text = open(logs[0]).read()
    assert "validation of epoch 0" in text and "emd:" in text and "> loss:" in text
    # a second run (epoch given: no checkpoint lookup) gives the same numbers
    again = pipe.run_valid(epoch=0)
    _check_metrics(again, got)


def test_run_valid_through_run_pipeline_main_and_run_test(dev, tmp_path, monkeypatch):
    from dmcf_amd import pipelines, run_pipeline
    from dmcf_amd.utils import tf_checkpoint as tc

    def load_ckpt(self, path):  # (the TensorFlow checkpoint itself is not shipped: its weights, as npz, are)
        tc.load_into_model(self.model, _weights(), device=dev)
        return 0

    monkeypatch.setattr(pipelines.Simulator, "load_ckpt", load_ckpt)
    got = run_pipeline.main(["-c", _yaml(tmp_path / "a"), "--split", "valid",
                             "--dataset_path", GOLDEN])
    assert set(got) == REF_KEYS
    args, extra = run_pipeline.parse_args(["-c", _yaml(tmp_path), "--split", "valid", "--dataset_path", GOLDEN])
    pipe = run_pipeline.build(args, extra)
    tc.load_into_model(pipe.model, _weights(), device=dev)
    _check_metrics(got, _expected(pipe, dev))
    # run_test with test_compute_metric: the rollouts are written, then run_valid(epoch) runs on the same split
    yml = _yaml(tmp_path / "b", extra_pipeline=dict(test_compute_metric=True))
    args, extra = run_pipeline.parse_args(["-c", yml, "--split", "test", "--dataset_path", GOLDEN])
    pipe = run_pipeline.build(args, extra)
    tc.load_into_model(pipe.model, _weights(), device=dev)
    paths = pipe.run_test(epoch=3)
    assert len(paths) == 1 and os.path.exists(paths[0])
    assert set(pipe.valid_loss) == REF_KEYS
    for k in REF_KEYS:
        assert abs(pipe.valid_loss[k] - got[k]) <= TOL[k] * max(abs(got[k]), 1e-3), k
    logs = glob.glob(os.path.join(pipe.cfg.logs_dir, "log_valid_*.txt"))
    assert len(logs) == 1 and "validation of epoch 3" in open(logs[0]).read()
    with pytest.raises(NotImplementedError):
        run_pipeline.main(["-c", yml, "--split", "train"])
