"""The forward CConv dispatch against its recorded snapshot (tests/golden/cconv_dispatch.json, written by
tests/golden/make_cconv_dispatch.py on a build of the commit named in the file): for every row the library must give the same
return code and string from dmcf_cconv_kernel_name / dmcf_cconv_extents_kernel_name and the same dmcf_cconv_workspace_bytes.
One intended difference: with DMCF_FLAG_SKIP_SELF, dmcf_cconv_kernel_name answers what dmcf_cconv_forward would --
DMCF_EUNSUPPORTED unless the direct kernel takes the call -- where the recorded commit named a kernel that is never launched.
No GPU: the queries only look at the arguments."""
import json
import os

import pytest

import cconv_dispatch_ref as dr
from dmcf_amd import ops

EUNSUPPORTED = -4
FAMILIES = ("cconv_direct_kernel", "cconv_ws_kernel", "cconv_pair_kernel", "cconv_p16_kernel", "cconv_z3_kernel", "cconv_cls_kernel",
            "cconv_blk_kernel", "cconv_mfma_kernel", "cconv_kernel")


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def snapshot():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cconv_dispatch.json")) as f:
        s = json.load(f)
    assert tuple(s["columns"]) == dr.INPUTS + dr.OUTPUTS
    ni = len(dr.INPUTS)
    name = lambda i: None if i < 0 else s["names"][i]  # noqa: E731
    return [(dict(zip(dr.INPUTS, r[:ni])), [r[ni], name(r[ni + 1]), r[ni + 2], name(r[ni + 3]), r[ni + 4]]) for r in s["rows"]]


def _family(name):
    return name and name.split("<")[0]


def test_snapshot_covers_the_dispatch(snapshot):
    """Every kernel family is in the file picked by the auto-rules (splat G, never auto-picked, excepted) and forced, every value
    of every axis of the grid occurs, and the SKIP_SELF rows hold both outcomes."""
    auto = {_family(want[1]) for row, want in snapshot if row["kernel"] is None and want[1]}
    forced = {_family(want[1]) for row, want in snapshot if row["kernel"] is not None and want[1]}
    assert auto == set(FAMILIES) - {"cconv_p16_kernel"}
    assert forced == set(FAMILIES)
    assert {_family(want[3]) for _, want in snapshot if want[3]} == {"cconv_ext_kernel"}
    seen = {k: {row[k] for row, _ in snapshot} for k in dr.INPUTS}
    assert seen["cin"] == {1, 3, 4, 8, 12, 16, 17, 24, 32, 36} and seen["cout"] == {1, 3, 4, 16, 17, 32, 33, 64, 65}
    assert {(r["d0"], r["d1"], r["d2"], r["sym_axis"]) for r, _ in snapshot} == {
        (4, 4, 4, -1), (1, 8, 8, -1), (1, 8, 1, -1), (3, 5, 2, -1), (6, 6, 6, -1), (4, 4, 2, 2), (6, 3, 6, 1)}
    assert seen["hint"] == {0, 1, 2} and seen["mapping"] == {0, 1, 2} and seen["interp"] == {0, 1, 2}
    assert seen["kind"] == {0, 1, 2} and seen["misaligned"] == {0, 1} and seen["split"] == {0, 1}
    for flag in (ops.FLAG_ALIGN_CORNERS, ops.FLAG_NORMALIZE, ops.FLAG_SKIP_SELF, ops.FLAG_ACCUMULATE):
        assert {bool(f & flag) for f in seen["flags"]} == {False, True}
    assert seen["n_out"] == {100, 16384, 20000} and {n for n in seen["n_inp"]} >= {2420, 1 << 24}
    assert any(r["n_inp"] < (1 << 24) and r["n_inp"] * r["cin"] * 4 >= (1 << 31) for r, _ in snapshot)
    assert seen["kernel"] == {None, "lds", "mfma", "blk", "cls", "z3", "pair", "ws", "g16", "direct", "bogus"}
    skip = [want for row, want in snapshot if row["flags"] & ops.FLAG_SKIP_SELF]
    assert any(_family(w[1]) == "cconv_direct_kernel" for w in skip) and any(_family(w[1]) != "cconv_direct_kernel" for w in skip)


def test_dispatch_reproduces_the_snapshot(hip_lib, monkeypatch, snapshot):
    bad = []
    for row, want in snapshot:
        got = dr.query(hip_lib, row, monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False))
        if (row["flags"] & ops.FLAG_SKIP_SELF) and want[0] == 0 and _family(want[1]) != "cconv_direct_kernel":
            want = [EUNSUPPORTED, None] + want[2:]
        if got != want:
            bad.append((row, want, got))
    assert not bad, f"{len(bad)} of {len(snapshot)} rows differ, the first: {bad[:3]}"
