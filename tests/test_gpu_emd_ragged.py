"""The ragged EMD on the GPU: dmcf_emd_ragged against dmcf_emd on every item alone (bit for bit), against the float64
restatement of tests/metrics_ref.py, emd_loss with row splits, and the one call per frame of valid_losses_batched.

Shapes.  One batch of items (n, m), in this order: (1, 1), (7, 3), (3, 7) -- both branches of the multipliers and their integer
division; (63, 65), (256, 257) -- the edges of a 256-row block and of a 256-point tile; (0, 0); (300, 700), whose split plan
has 3 chunks of 256 columns one way and 2 the other; (0, 5), (5, 0) -- one set empty, cost 0; (2025, 2025), the validation
workload's scene, 8 x 8 splits; and last (20000, 7000), whose chunks are two tiles long (14 chunks of 512 columns one way, 40
the other).  Points are uniform in the unit cube, as in tests/test_gpu_metrics.py."""
import tempfile
import types

import numpy as np
import pytest

import metrics_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(1, 1), (7, 3), (3, 7), (63, 65), (256, 257), (0, 0), (300, 700), (0, 5), (5, 0), (2025, 2025), (20000, 7000)]


def _splits(counts):
    rs = [0]
    for c in counts:
        rs.append(rs[-1] + c)
    return rs


def test_the_plans_the_shapes_were_chosen_for():
    """mt_plan of csrc/metrics_plan.h restated (batch 1): the chunk counts and lengths the module's docstring names."""
    def plan(rows, cols):
        row_blocks, tiles = -(-rows // 256), max(-(-cols // 256), 1)
        ns = max(min(-(-2048 // row_blocks), tiles), 1)
        per = -(-tiles // ns)
        return -(-tiles // per), per * 256
    assert plan(300, 700) == (3, 256) and plan(700, 300) == (2, 256)
    assert plan(2025, 2025) == (8, 256)
    assert plan(20000, 7000) == (14, 512) and plan(7000, 20000) == (40, 512)


@pytest.fixture(scope="module")
def ragged():
    """The batch, the ragged call's costs and ops.emd on every item alone (the parent's code), computed once."""
    from dmcf_amd import ops
    rng = np.random.default_rng(24)
    a = [rng.uniform(0, 1, size=(n, 3)).astype(np.float32) for n, _ in SIZES]
    b = [rng.uniform(0, 1, size=(m, 3)).astype(np.float32) for _, m in SIZES]
    rs1, rs2 = _splits([n for n, _ in SIZES]), _splits([m for _, m in SIZES])
    A, B = torch.from_numpy(np.concatenate(a)).to(DEV), torch.from_numpy(np.concatenate(b)).to(DEV)
    got = ops.emd_ragged(A, B, rs1, rs2)
    one = torch.zeros(1, 1, 3, device=DEV)  # (an empty set reaches dmcf_emd as a zero count over a point that plays no part)
    per_item = [ops.emd(A[rs1[k]:rs1[k + 1]][None], B[rs2[k]:rs2[k + 1]][None])[0] if n and m else
                ops.emd(A[rs1[k]:rs1[k + 1]][None] if n else one, B[rs2[k]:rs2[k + 1]][None] if m else one, [n], [m])[0]
                for k, (n, m) in enumerate(SIZES)]
    return dict(a=a, b=b, A=A, B=B, rs1=rs1, rs2=rs2, got=got, per_item=per_item)


def test_every_item_has_the_per_item_calls_bits(ragged):
    got = ragged["got"]
    assert got.shape == (len(SIZES),) and got.dtype == torch.float32 and got.device.type == "cuda"
    print("ragged  ", got.tolist())
    print("per item", [float(x) for x in ragged["per_item"]])
    for k, want in enumerate(ragged["per_item"]):
        assert torch.equal(got[k], want), (k, SIZES[k], float(got[k]), float(want))
    for k, (n, m) in enumerate(SIZES):
        assert (float(got[k]) == 0.0) == (n == 0 or m == 0), (k, float(got[k]))


def test_repeatable_and_the_forms_of_the_splits(ragged):
    from dmcf_amd import ops
    A, B, rs1, rs2 = ragged["A"], ragged["B"], ragged["rs1"], ragged["rs2"]
    assert torch.equal(ops.emd_ragged(A, B, rs1, rs2), ragged["got"])
    # a CPU tensor, a device tensor; ops.emd dispatches on the splits
    cpu = [torch.tensor(rs, dtype=torch.int64) for rs in (rs1, rs2)]
    assert torch.equal(ops.emd(A, B, row_splits1=cpu[0], row_splits2=cpu[1]), ragged["got"])
    assert torch.equal(ops.emd(A, B, row_splits1=cpu[0].to(DEV), row_splits2=cpu[1].to(DEV)), ragged["got"])


def test_permuting_the_items_permutes_the_costs(ragged):
    from dmcf_amd import ops
    order = [10, 3, 8, 0, 9, 5, 1, 7, 6, 2, 4]
    assert sorted(order) == list(range(len(SIZES)))
    a, b = [ragged["a"][k] for k in order], [ragged["b"][k] for k in order]
    got = ops.emd_ragged(torch.from_numpy(np.concatenate(a)).to(DEV), torch.from_numpy(np.concatenate(b)).to(DEV),
                         _splits([len(x) for x in a]), _splits([len(x) for x in b]))
    assert torch.equal(got, ragged["got"][torch.tensor(order, device=DEV)])


def test_2d_sets_equal_the_padded_call(ragged):
    from dmcf_amd import ops
    sizes = SIZES[:9]
    rs1, rs2 = _splits([n for n, _ in sizes]), _splits([m for _, m in sizes])
    A2, B2 = ragged["A"][:rs1[-1], :2].contiguous(), ragged["B"][:rs2[-1], :2].contiguous()
    got = ops.emd_ragged(A2, B2, rs1, rs2)
    pad = torch.nn.functional.pad
    assert torch.equal(got, ops.emd_ragged(pad(A2, (0, 1)), pad(B2, (0, 1)), rs1, rs2))
    assert got.shape == (9,) and float(got[6]) > 0.0 and not torch.equal(got[6], ragged["got"][6])  # (z took part above)


def test_against_float64(ragged):
    """match_cost(approx_match(...)) of tests/metrics_ref.py in float64 on every item but the last (20000 x 7000 float64 pairs
    are too many for the restatement), held to the bar tests/test_gpu_metrics.py holds ops.emd to."""
    got = ragged["got"].cpu().numpy().astype(np.float64)
    for k, (n, m) in enumerate(SIZES[:-1]):
        if n == 0 or m == 0:
            assert got[k] == 0.0
            continue
        a, b = ragged["a"][k][None], ragged["b"][k][None]
        want = metrics_ref.match_cost(a, b, metrics_ref.approx_match(a, b))
        e = got[k:k + 1]
        print(f"item {k} {SIZES[k]}: emd {e[0]:.9g}, float64 {want[0]:.9g}, |diff| / (1e-4 want) = "
              f"{abs(e[0] - want[0]) / (1e-4 * want[0]):.3f}")
        assert np.abs(e - want).max() <= 1e-4 * want.max(), (k, e, want)


def test_emd_loss_with_splits(ragged):
    from dmcf_amd.utils.tools.losses import emd_loss
    A, B, rs1, rs2 = ragged["A"], ragged["B"], ragged["rs1"], ragged["rs2"]
    got = emd_loss(A, B, true_row_splits=rs1, pred_row_splits=rs2)
    assert got.shape == (len(SIZES),) and got.dtype == torch.float32
    for k, (n, m) in enumerate(SIZES):
        if n == 0 and m == 0:
            assert float(got[k]) == 0.0  # (the per-item call divides 0 by 0 here)
            continue
        x, y = A[rs1[k]:rs1[k + 1]][None], B[rs2[k]:rs2[k + 1]][None]
        one = torch.zeros(1, 1, 3, device=DEV)  # (an empty set: a zero count, as in the fixture)
        want = emd_loss(x, y)[0] if n and m else emd_loss(x if n else one, y if m else one, n=[n], m=[m])[0]
        assert torch.equal(got[k], want), (k, float(got[k]), float(want))
    # every item empty: zeros, without a launch
    none = emd_loss(A[:0], B[:0], true_row_splits=[0, 0, 0], pred_row_splits=[0, 0, 0])
    assert none.shape == (2,) and not none.any()


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


def test_valid_losses_batched_makes_one_call_per_frame(monkeypatch):
    """Two scenes, three frames (two evaluated): one dmcf_emd_ragged call per frame, no dmcf_emd call, and every scene's
    ``emd`` the per-scene emd_loss of the loop on the same clamped positions, bit for bit."""
    from test_gpu_step_batched import _model
    from test_gpu_valid_batched import _scenes
    from dmcf_amd import _lib
    from dmcf_amd.pipelines.simulator import Simulator
    from dmcf_amd.utils.tools.losses import emd_loss
    data = _scenes((0, 2), 3)
    sim = Simulator(_model("waterramps"), dataset=types.SimpleNamespace(valid=None), device="cuda", main_log_dir=tempfile.mkdtemp(),
                    split="valid", valid_batched=True)
    results = sim.run_rollout_batched(data, 3)
    counting = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    losses = sim.valid_losses_batched(data, results)
    assert counting.calls.get("dmcf_emd_ragged", 0) == 2 and counting.calls.get("dmcf_emd", 0) == 0
    for i, d in enumerate(data):
        lo, hi = (torch.from_numpy(f(d["box"][0], axis=0)).to(DEV) for f in (np.min, np.max))
        for t in (1, 2):
            pos = torch.clamp(results[i][t][0], lo, hi)
            tgt = torch.from_numpy(d["pos"][t]).to(DEV)
            want = float(np.mean(emd_loss(tgt.unsqueeze(0), pos.unsqueeze(0)).cpu().numpy().astype(np.float32)))
            assert losses[i][t]["emd"] == want and want > 0.0, (i, t, losses[i][t]["emd"], want)
