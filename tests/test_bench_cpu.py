"""bench.py's host side without a GPU: the argument checks and what --dump-outputs writes."""
import numpy as np
import pytest

import bench


def test_steps_and_dump_arguments():
    a = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "out"
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "out"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_full_argument():
    """--full is off by default; the options that only size or record its extra measurements need it."""
    assert not bench.parse_args([]).full and bench.parse_args(["--full"]).full
    assert bench.parse_args(["--full", "--cpu-side", "8"]).cpu_side == 8
    assert bench.parse_args(["--cpu-side", "0"]).cpu_side == 0
    assert bench.parse_args(["--layers-json", "l.json"]).layers_json == "l.json"
    assert bench.parse_args(["--full", "--config", "wbcsph", "--layers-json", "l.json"]).full
    for bad in (["--cpu-side", "8"], ["--config", "wbcsph", "--layers-json", "l.json"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_whole_and_sampled(tmp_path):
    rng = np.random.default_rng(5)
    pos, vel = rng.normal(size=(1000, 3)), rng.normal(size=(1000, 3)).astype(np.float32)
    d = bench.dump_outputs(str(tmp_path / "all"), dict(pos=pos, vel=vel))
    assert d["rows"] == d["of_rows"] == 1000 and d["sample"] is None
    for name, ref in (("pos", pos), ("vel", vel)):
        a = np.load(tmp_path / "all" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, ref.astype(np.float32))
    # beyond the limit: the same seeded rows of every array, the files within the limit, the same rows on every call
    limit = 10_000
    for run in ("s1", "s2"):
        d = bench.dump_outputs(str(tmp_path / run), dict(pos=pos, vel=vel), limit=limit)
        assert d["of_rows"] == 1000 and 0 < d["rows"] < 1000 and d["sample"]
        assert sum((tmp_path / run / f"{n}.npy").stat().st_size for n in ("pos", "vel")) <= limit
        keep = np.sort(np.random.default_rng(0).choice(1000, d["rows"], replace=False))
        for name, ref in (("pos", pos), ("vel", vel)):
            assert np.array_equal(np.load(tmp_path / run / f"{name}.npy"), ref.astype(np.float32)[keep])
    assert (tmp_path / "s1" / "pos.npy").read_bytes() == (tmp_path / "s2" / "pos.npy").read_bytes()
