"""run_valid with ``valid_batched``: the two ``vel_diff_val*`` from ONE dmcf_hist_pair_ragged call per evaluated frame, against
the per-scene loop's host compare_dist -- bit for bit, on the two-scene, three-frame in-memory split of
tests/test_gpu_valid_batched.py (its scenes, model and counting library, taken over as they are).  The batched metrics run on
the LOOPED rollout's results (as that file's ``staged`` run does), so both sides histogram the same velocities."""
import tempfile
import types

import numpy as np
import pytest

from test_gpu_valid_batched import _Counting, _scenes, model  # noqa: F401  (model: the module-scoped fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FRAMES = 2  # evaluated frames of a three-frame split (t = 1, 2)


@pytest.fixture(scope="module")
def runs(model):  # noqa: F811
    """Looped and batched run_valid on float32 velocities and on float64 ones, all four on one rollout; the batched runs
    under the counting library, the float32 one with evaluation_helper.compare_dist replaced by a function that raises."""
    from dmcf_amd import _lib, datasets
    from dmcf_amd.pipelines.simulator import Simulator
    from dmcf_amd.utils import evaluation_helper
    data = _scenes((0, 2), 3)
    data64 = [dict(d, vel=d["vel"].astype(np.float64)) for d in data]
    mp = pytest.MonkeyPatch()
    res, current, kept = {}, [data], []
    try:
        mp.setattr(datasets, "get_rollout", lambda *a, **k: current[0])

        def sim(**kw):
            return Simulator(model, dataset=types.SimpleNamespace(valid=None), device="cuda", main_log_dir=tempfile.mkdtemp(),
                             split="valid", **kw)
        looped = sim()
        rollout = looped.run_rollout
        looped.run_rollout = lambda *a: kept.append(rollout(*a)) or kept[-1]
        res["looped"] = dict(looped.run_valid(epoch=0))
        counting = _Counting(_lib.lib())
        mp.setattr(_lib, "lib", lambda: counting)
        host_calls = []
        real = evaluation_helper.compare_dist

        def refuse(*a, **k):
            raise AssertionError("compare_dist was called: the batched validation histograms on the device")

        def counted(*a, **k):
            host_calls.append(1)
            return real(*a, **k)

        def staged():
            s = sim(valid_batched=True)
            s.run_rollout_batched = lambda *a: kept[0]
            counting.calls.clear()
            return dict(s.run_valid(epoch=0)), dict(counting.calls)
        mp.setattr(evaluation_helper, "compare_dist", refuse)
        res["batched"], res["batched_calls"] = staged()
        # float64 target velocities (the rollout casts its inputs to float32, so the results are the same)
        current[0] = data64
        mp.setattr(evaluation_helper, "compare_dist", real)
        looped64 = sim()
        looped64.run_rollout = lambda *a: kept[0]
        res["looped64"] = dict(looped64.run_valid(epoch=0))
        mp.setattr(evaluation_helper, "compare_dist", counted)
        res["batched64"], res["batched64_calls"] = staged()
        res["host_calls64"] = len(host_calls)
    finally:
        mp.undo()
    return res


def test_vel_diff_val_has_the_loops_bits(runs):
    want, got = runs["looped"], runs["batched"]
    print("looped ", want["vel_diff_val"], want["vel_diff_val_2"])
    print("batched", got["vel_diff_val"], got["vel_diff_val_2"])
    assert list(got) == list(want)
    assert np.isfinite(want["vel_diff_val"]) and want["vel_diff_val"] != want["vel_diff_val_2"]
    assert got["vel_diff_val"] == want["vel_diff_val"] and got["vel_diff_val_2"] == want["vel_diff_val_2"]


def test_one_call_per_frame_and_no_host_histogram(runs):
    # (the fixture's compare_dist raises, so reaching this point already shows zero host calls)
    assert runs["batched_calls"].get("dmcf_hist_pair_ragged", 0) == FRAMES
    assert runs["batched_calls"].get("dmcf_hist_pair_ragged_workspace_bytes", 0) == FRAMES


def test_float64_velocities_keep_the_host_path(runs):
    want, got = runs["looped64"], runs["batched64"]
    assert got["vel_diff_val"] == want["vel_diff_val"] and got["vel_diff_val_2"] == want["vel_diff_val_2"]
    assert runs["batched64_calls"].get("dmcf_hist_pair_ragged", 0) == 0
    assert runs["host_calls64"] == 2 * FRAMES * 2  # (scenes x frames x directions)
