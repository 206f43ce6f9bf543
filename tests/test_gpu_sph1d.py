"""dmcf_sph1d_rollout on the GPU (dmcf_amd/csrc/sph1d.hip) and the column generator on top of it, against the scenes the
REFERENCE's generator produced (tests/golden/column_gen.npz, tests/golden/column_test.npz): the error bar of
tests/column_gen_bar.py, the iteration counts, bit-equality of cut and batched rollouts, the 64-point limit, and the generated
test split through DatasetGroup and run_pipeline."""
import os

import numpy as np
import pytest
import torch

import column_gen_bar as bar

pytestmark = pytest.mark.gpu
GOLDEN = bar.GOLDEN
HRNET_DATASET = dict(name="Column2", type="column", **bar.DATASET, train=dict(seed=42, min_pts=1, max_pts=40, data_cnt=40, timesteps=100),
                     valid=dict(seed=43, min_pts=1, max_pts=40, data_cnt=10, timesteps=100),
                     test=dict(seed=44, offset=10.0, pts_cnt=[1, 5], data_cnt=2, timesteps=200))  # configs/column/hrnet.yml:1-32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _states(name):
    from dmcf_amd.datasets import column_gen
    seed, sec = bar.CASES[name]
    kw = {k: v for k, v in sec.items() if k in ("data_cnt", "min_pts", "max_pts", "pts_cnt", "rnd", "offset")}
    np.random.seed(seed)
    return column_gen.draw_states(**kw)[1]


def _constants():
    from dmcf_amd.datasets import column_gen
    return column_gen.solver_constants(gravity=bar.DATASET["gravity"] * bar.DATASET["res"], dt=bar.DATASET["dt"])


def _batch(states, dev):
    n = [len(s) for s in states]
    b = np.zeros((len(states), max(n), 3), np.float32)
    for s, st in enumerate(states):
        b[s, :len(st)] = st
    return torch.from_numpy(b).to(dev), n


@pytest.fixture(scope="module")
def runs(dev):
    """Every case generated once through the product's gen_data hooks: name -> (scenes, per-scene iteration counts)."""
    from dmcf_amd.datasets import column_gen
    out = {}
    for name, (seed, sec) in bar.CASES.items():
        np.random.seed(seed)
        gravity = bar.DATASET["gravity"] * bar.DATASET["res"]
        states = column_gen.draw_states(**{k: v for k, v in sec.items() if k != "timesteps"})[1]
        seqs, iters = column_gen.rollout(states, sec["timesteps"], **column_gen.solver_constants(gravity=gravity, dt=bar.DATASET["dt"]))
        scenes = [column_gen.gen_dict(np.ascontiguousarray(q[:, ::-1]), d, bar.DATASET["res"], 2, gravity) for d, q in enumerate(seqs)]
        out[name] = (scenes, iters)
    return out


@pytest.mark.parametrize("name", sorted(bar.CASES))
def test_kernel_meets_the_bar(runs, name):
    scenes, _ = runs[name]
    assert len(scenes) == int(bar.fixture()[f"{name}_scenes"])
    for s, scene in enumerate(scenes):
        bar.check_scene(name, s, np.stack([f["pos"] for f in scene]), np.stack([f["vel"] for f in scene]))


def test_gen_data_is_what_the_hooks_give(runs):
    """gen_data itself (seeded as DatasetGroup seeds it; case c, the random draws) returns the scenes of draw_states -> rollout
    -> gen_dict, bit for bit."""
    from dmcf_amd.datasets import column_gen
    seed, sec = bar.CASES["c"]
    np.random.seed(seed)
    data = column_gen.gen_data(**sec, **bar.DATASET)
    assert len(data) == len(runs["c"][0])
    for scene, ours in zip(data, runs["c"][0]):
        assert len(scene) == len(ours)
        for f, g in zip(scene, ours):
            assert list(f) == list(g)
            for k in ("pos", "vel", "box", "box_normals", "grav"):
                np.testing.assert_array_equal(f[k], g[k])


def test_iteration_counts(runs, dev):
    """Counts lie in [1, max_iter].  A lone particle in free flight converges in its first iteration on every step: in case a's
    1-particle scene those are the steps before it reaches the boundary (the reference's own counts there are 1; after the
    contact near frame 56 the reference iterates up to 2238 times, so 'every step' holds for the flight only), and a
    1-particle scene that never lands shows it for a whole rollout."""
    from dmcf_amd import ops
    fx = bar.fixture()
    for name, (_, iters) in runs.items():
        for s, it in enumerate(iters):
            ref = fx[f"{name}_s{s}_iters"]
            print(f"case {name} scene {s}: iterations {it.min()}..{it.max()} sum {it.sum()}  (reference {ref.min()}..{ref.max()} sum {ref.sum()})")
            assert it.dtype == np.int32 and it.shape == ref.shape and it.min() >= 1 and it.max() <= 10000
    flight = fx["a_s0_iters"] == 1
    assert flight[:50].all()
    np.testing.assert_array_equal(runs["a"][1][0][flight], 1)
    state = torch.tensor([[[0.0, 0.0, 1.0], [0.5, 0.0, 1.0], [1000.0, 0.0, 1.0]]], device=dev)
    _, _, iters = ops.sph1d_rollout(state, [3], 40, **_constants())
    assert (iters == 1).all()


def test_cut_rollout_equals_single_launch(dev):
    from dmcf_amd import ops
    state, n = _batch(_states("c") + _states("b"), dev)
    c = _constants()
    one = ops.sph1d_rollout(state, n, 5, launch_iters=10 ** 9, **c)
    for per_launch in (1, 2):
        cut = ops.sph1d_rollout(state, n, 5, launch_iters=per_launch * c["max_iter"], **c)
        for a, b in zip(one, cut):
            assert torch.equal(a, b)
    assert torch.equal(state, _batch(_states("c") + _states("b"), dev)[0])  # the caller's state is not advanced in place


def test_batch_equals_scenes_one_at_a_time(dev):
    from dmcf_amd import ops
    states = _states("c") + _states("a") + _states("b")
    state, n = _batch(states, dev)
    c = _constants()
    seq, out, iters = ops.sph1d_rollout(state, n, 4, **c)
    assert seq.shape == (4, len(states), max(n), 2) and out.shape == state.shape and iters.shape == (4, len(states))
    for s, st in enumerate(states):
        q, o, it = ops.sph1d_rollout(torch.from_numpy(st).to(dev)[None], [n[s]], 4, **c)
        assert torch.equal(q[:, 0], seq[:, s, :n[s]]) and torch.equal(o[0], out[s, :n[s]]) and torch.equal(it[:, 0], iters[:, s])
        assert (seq[:, s, n[s]:] == 0).all()  # padding slots are written as zeros


def test_65_points_are_refused(dev):
    from dmcf_amd import ops
    state = torch.zeros((1, 65, 3), device=dev)
    with pytest.raises(NotImplementedError, match="64"):
        ops.sph1d_rollout(state, [65], 1, **_constants())
    from dmcf_amd.datasets import column_gen
    with pytest.raises(NotImplementedError, match="64"):
        column_gen.gen_data(data_cnt=1, timesteps=1, pts_cnt=[63], **bar.DATASET)
    seq, _, _ = ops.sph1d_rollout(torch.zeros((1, 64, 3), device=dev), [0], 1, **_constants())  # 64 slots are accepted
    assert seq.shape == (1, 1, 64, 2)


def test_dataset_group_generates_the_hrnet_test_split(dev, tmp_path):
    """DatasetGroup(**hrnet.yml's dataset section, split='test') against the reference's two test scenes
    (tests/golden/column_test.npz), frames 0-99 under case a's bar; then a second group reads the cache."""
    from dmcf_amd.datasets import DatasetGroup
    g = DatasetGroup(**HRNET_DATASET, split="test", cache_dir=str(tmp_path / "cache"))
    assert g.train is None and g.valid is g.test and len(g.test) == 2
    fix = np.load(os.path.join(GOLDEN, "column_test.npz"))
    fx = bar.fixture()
    for s in (0, 1):
        scene = g.test[s]
        assert len(scene) == 200 and [f["frame_id"] for f in scene] == list(range(200)) and scene[0]["scene_id"] == "sim_%04d" % s
        np.testing.assert_array_equal(fix[f"s{s}_pos"][:100], fx[f"a_s{s}_pos"])  # the two fixtures agree on what case a is
        bar.check_scene("a", s, np.stack([f["pos"] for f in scene[:100]]), np.stack([f["vel"] for f in scene[:100]]))
        np.testing.assert_array_equal(scene[0]["box"], fix[f"s{s}_box"])
        np.testing.assert_array_equal(scene[0]["box_normals"], fix[f"s{s}_box_normals"])
        np.testing.assert_array_equal(scene[7]["grav"], fix[f"s{s}_grav"][7].astype(np.float64))
        assert np.isfinite(np.stack([f["pos"] for f in scene])).all()
    again = DatasetGroup(**HRNET_DATASET, split="test", cache_dir=str(tmp_path / "cache"))
    for f, h in zip(g.test[1], again.test[1]):
        np.testing.assert_array_equal(f["pos"], h["pos"])
        np.testing.assert_array_equal(f["vel"], h["vel"])


def test_run_pipeline_test_split_on_generated_scenes(dev, tmp_path):
    """run_pipeline --split test on a config WITHOUT a dataset_path: the column test split is generated, rolled out by the
    column HRNet (tools/configs.py; its initialisers, no checkpoint) and written."""
    import yaml
    from dmcf_amd import run_pipeline
    from tools import configs
    cfg = dict(dataset=dict(HRNET_DATASET, cache_dir=str(tmp_path / "cache")), model=dict(configs.COLUMN_HRNET, ckpt_path=None),
               pipeline=dict(name="Simulator", version="v0", main_log_dir=str(tmp_path / "logs"), output_dir=str(tmp_path / "out"),
                             data_generator=dict(translate=[0.0, 0.0, 0.0], scale=[0.0, 1.0, 0.0], train=dict(stride=1),
                                                 valid=dict(stride=1), test=dict(stride=1, time_end=4))))
    yml = tmp_path / "column.yml"
    yml.write_text(yaml.safe_dump(cfg))
    paths = run_pipeline.main(["-c", str(yml), "--split", "test"])
    assert len(paths) == 2 and all(os.path.getsize(p) > 0 for p in paths)
    assert os.path.isdir(tmp_path / "cache")
