"""The routes of ``dmcf_amd/utils/convolutions.py`` that a CPU tensor never takes, call by call on the GPU: the lattice form with
and without stray rows, the scatter form, the ASCC head on the trunk's list (skip_self), the ``_direct_kernel`` query with its
announcement, and a recording step with record_lattice_form and record_scatter_form -- against the transcript recorded before
the call preparation was folded (tests/golden/conv_transcript_gpu.json, a digest per record; recorder:
tests/conv_transcript.py; the CPU routes: tests/test_conv_transcript_cpu.py).

Scene: tools.scenes.box_scene(12) with SCATTER_MIN_INPUTS = 256 (where tests/test_gpu_scatter_training.py gets splat S), the
Liquid3d config with the reference's weights, two Simulator steps and then one recording forward; once as it is and once with
three particles moved out of the box and every lattice split into a core and stray rows.

The tensors of the arguments in NO_CRC are recorded without their CRC: the raw list buffers, whose tails past the rows are
never written, and the packed-filter workspace -- what differed between three runs of the same code when the golden was
captured; every other CRC was equal in all three (``DMCF_CAPTURE_TRANSCRIPTS=1 pytest tests/test_gpu_conv_transcript.py``
rewrites the golden)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_transcript as ct  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN_FILE = "conv_transcript_gpu.json"
NO_CRC = ("neighbors_index", "neighbors_value", "t_index", "packed_cache")


def _variant(strays):
    from dmcf_amd import lattice
    from dmcf_amd.pipelines import Simulator
    from dmcf_amd.utils import convolutions
    from test_gpu_model import GOLDEN, _build
    from tools import configs, scenes
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(convolutions, "SCATTER_MIN_INPUTS", 256)
        mp.setattr(convolutions, "_CACHE", convolutions._PerThreadCache())  # (no estimates from another test's steps)
        lattice._cores().clear()
        scene = scenes.box_scene(12)
        if strays:
            mp.setattr(lattice, "CORE_MIN_FILL", 2.0)  # (above any fill: every lattice is split into its core and stray rows)
            scene["pos"][:3] += np.float32([[1.5, 0.7, 0.0], [0.0, 1.1, 0.9], [-1.3, 0.0, 0.4]])
        model = _build(configs.LIQUID3D, dict(np.load(os.path.join(GOLDEN, "liquid3d_weights.npz"))), torch.device("cuda:0"))
        sim = Simulator(model, device="cuda")
        state = scenes.model_inputs(scene, device="cuda:0")
        rec = ct.Recorder(mp, no_crc=NO_CRC)
        for step in (1, 2):
            state = sim.step([state])[0]
            rec.records.append({"step": step, "consumers": sorted(repr(kv) for kv in convolutions._CACHE.expect.items())})
        model.requires_grad_(True)
        model.record_lattice_form(True)
        model.record_scatter_form(True)
        model(scenes.model_inputs(scene, device="cuda:0"))
        rec.records.append({"step": "recording"})
        torch.cuda.synchronize()
        return rec.records
    finally:
        mp.undo()


def _transcripts():
    return {"box": _variant(False), "strays": _variant(True)}


@pytest.fixture(scope="module")
def golden():
    if os.environ.get("DMCF_CAPTURE_TRANSCRIPTS") == "1":
        ct.dump(_transcripts(), os.path.join(ct.GOLDEN, GOLDEN_FILE))
    return ct.load(GOLDEN_FILE)


@pytest.fixture(scope="module")
def got():
    return _transcripts()


@pytest.mark.parametrize("variant", ["box", "strays"])
def test_transcript_equals_the_recorded_one(variant, golden, got):
    assert ct.first_difference(golden[variant], got[variant]) is None


def _steps(records):
    """-> {step: its records}."""
    out, cur = {}, []
    for r in records:
        if "step" in r:
            out[r["step"]], cur = cur, []
        else:
            cur.append(r)
    return out


def _calls(records, name):
    return [r["args"] for r in records if r.get("call") == name]


def test_the_transcript_takes_every_route(got):
    """Otherwise the comparison above would pin the neighbour-list route only."""
    box, strays = _steps(got["box"]), _steps(got["strays"])
    for step in (1, 2):
        assert _calls(box[step], "lattice_conv") and _calls(box[step], "cconv_scatter_forward") and _calls(box[step], "scatter_plan")
        assert not [a for a in _calls(box[step], "cconv_forward") if a.get("row_length_hint") == 1 and "normalize" not in a]
        # the stray rows of a split lattice: the call without normalize / symmetric, right after the stencil launch
        assert [a for a in _calls(strays[step], "cconv_forward") if a.get("row_length_hint") == 1 and "normalize" not in a]
    # the ASCC head: asked once which kernel serves it, announced as a consumer, and from the second step on the trunk's list
    assert len([a for a in _calls(box[1], "cconv_forward") if a.get("name_only")]) == 1
    assert not [a for a in _calls(box[2], "cconv_forward") if a.get("name_only")]
    assert not [a for a in _calls(box[1], "cconv_forward") if a.get("skip_self")]
    assert len([a for a in _calls(box[2], "cconv_forward") if a.get("skip_self")]) == 1
    assert len(_calls(box[2], "fixed_radius_search")) == len(_calls(box[1], "fixed_radius_search")) - 1
    heads = [r for r in box[1] if r.get("after", {}).get("_direct_kernel") is True]
    assert len(heads) == 1
    assert _calls(box["recording"], "ScatterConvFunction.apply") and _calls(box["recording"], "lattice_conv")
    assert _calls(box["recording"], "cconv_scatter_forward")


def test_the_announcement_adds_a_consumer(got):
    """The first step ends with one more consumer of the trunk's s0 -> s0 list than its layers took: the head's announcement."""
    steps = [r for r in got["box"] if r.get("step") in (1, 2)]
    assert steps[0]["consumers"] and steps[0]["consumers"] != steps[1]["consumers"]
