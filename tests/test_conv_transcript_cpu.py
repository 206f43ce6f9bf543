"""ContinuousConv and PointSampling on CPU tensors, call by call: which ``ops`` function every route of
``dmcf_amd/utils/convolutions.py`` calls, in which order, with which arguments, what the layer keeps afterwards, the bits of
the result and every refusal -- against the transcripts recorded before the call preparation was folded
(tests/golden/conv_transcript_cpu.json, a digest per record; recorder: tests/conv_transcript.py).  A failure prints the
record that departs in full.

Backend: tests/shims.py for the searches, plus what it lacks here -- the batched FixedRadiusSearch and the RadiusSearch (the
brute force of tests/batched_search_ref.py) and a ``cconv_forward`` in torch that autograd can record.  That stand-in is NOT
the operator (window-weighted neighbour sums through two of the filter's cells): the operands are pinned by the transcript, the
stand-in only makes the result depend on them and on the epilogue requests (bias, out, accumulate).

``DMCF_CAPTURE_TRANSCRIPTS=1 pytest tests/test_conv_transcript_cpu.py`` rewrites the golden file; only a change of behaviour
that is meant may do that."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_transcript as ct  # noqa: E402
import shims  # noqa: E402
from batched_search_ref import batched_brute_force  # noqa: E402
from dmcf_amd import ops  # noqa: E402
from dmcf_amd.utils import convolutions  # noqa: E402
from dmcf_amd.utils.convolutions import ContinuousConv, PointSampling, neighbor_cache  # noqa: E402
from dmcf_amd.utils.tools.losses import get_window_func  # noqa: E402

GOLDEN_FILE = "conv_transcript_cpu.json"
N_INP, N_OUT, CIN, COUT, EXTENT = 48, 36, 3, 4, 0.6


def callable_window(q):
    return torch.clamp(1 - q, 0, 1) ** 2


WINDOWS = {"named": lambda: get_window_func("poly6"), "callable": lambda: callable_window, "none": lambda: None}


def install_backend(monkeypatch):
    shims.install(monkeypatch)
    single = ops.fixed_radius_search

    def result(idx, rs, d, return_distances):
        d = torch.from_numpy(d) if return_distances else torch.empty(0)
        return ops.NeighborSearchResult(torch.from_numpy(idx), torch.from_numpy(rs), d, total=len(idx))

    def fixed_radius_search(points, queries, radius, ignore_query_point=False, return_distances=True, hash_table=None,
                            capacity_hint=None, row_stride=None, max_count=None, points_row_splits=None, queries_row_splits=None):
        if points_row_splits is None:
            return single(points, queries, radius, ignore_query_point, return_distances, hash_table)
        idx, rs, d = batched_brute_force(points.numpy(), queries.numpy(), radius, points_row_splits.numpy(),
                                         queries_row_splits.numpy(), ignore_query_point)
        return result(idx, rs, d, return_distances)

    def radius_search(points, queries, radii, ignore_query_point=False, return_distances=True, normalize_distances=True,
                      points_row_splits=None, queries_row_splits=None):
        n, m = points.shape[0], queries.shape[0]
        prs = np.array([0, n]) if points_row_splits is None else points_row_splits.numpy()
        qrs = np.array([0, m]) if queries_row_splits is None else queries_row_splits.numpy()
        idx, rs, d = batched_brute_force(points.numpy(), queries.numpy(), radii.numpy(), prs, qrs, ignore_query_point)
        if normalize_distances:
            d = d / np.repeat(radii.numpy() ** 2, np.diff(rs))
        return result(idx, rs, d.astype(np.float32), return_distances)

    def cconv_forward(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
                      neighbors_value=None, window=None, window_fac=1.0, inp_importance=None, bias=None, out=None,
                      accumulate=False, name_only=False, **geometry):
        if name_only:
            return "cconv_stand_in"
        n_out = out_positions.shape[0]
        index = neighbors_index.long()
        rows = torch.repeat_interleave(torch.arange(n_out), torch.diff(neighbors_row_splits))
        f = inp_features[index]
        if window == "explicit":
            f = f * neighbors_value[:, None]
        elif window is not None and neighbors_value is not None:
            f = f * (window_fac / (1 + neighbors_value[:, None]))
        if inp_importance is not None:
            f = f * inp_importance[index][:, None]
        # (element-wise products and sums in a fixed order only: no reduction or GEMM whose summation order the CPU chooses)
        cells = filters.reshape(-1, *filters.shape[-2:])
        w = cells[0] + cells[-1]
        per_channel = torch.zeros(n_out, f.shape[1]).index_add(0, rows, f)
        y = sum(per_channel[:, c:c + 1] * w[c] for c in range(w.shape[0]))
        if bias is not None:
            y = y + bias
        if out is None:
            return y
        return out.copy_(out + y if accumulate else y)

    monkeypatch.setattr(ops, "fixed_radius_search", fixed_radius_search)
    monkeypatch.setattr(ops, "radius_search", radius_search)
    monkeypatch.setattr(ops, "cconv_forward", cconv_forward)


def scene():
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    inp = t(rng.uniform(0, 1, (N_INP, 3)))
    out = t(rng.uniform(0, 1, (N_OUT, 3)))
    return dict(inp_positions=inp, out_positions=out, inp_features=t(rng.normal(size=(N_INP, CIN))),
                rank1=t(rng.uniform(0.4, 0.8, N_OUT)), importance=t(rng.uniform(0.5, 1.5, N_INP)),
                acc=t(rng.normal(size=(N_OUT, COUT))), acc_inp=t(rng.normal(size=(N_INP, COUT))), extra=t(rng.normal(size=COUT)))


def seeded_weights():
    """The three initializers of a layer, from numpy's generator (its streams are stable across versions)."""
    rng = np.random.default_rng(3)
    init = lambda shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32))  # noqa: E731
    return dict(kernel_initializer=init, bias_initializer=init, dense_kernel_initializer=init)


def layer(record, window="named", cls=ContinuousConv, **kw):
    if cls is PointSampling:
        return PointSampling(window_function=WINDOWS[window](), **kw)
    kw.setdefault("kernel_size", [4, 4, 4])
    conv = ContinuousConv(COUT, window_function=WINDOWS[window](), device="cpu", normalize=False, **seeded_weights(), **kw)
    conv.build(CIN, "cpu")
    if record:
        conv.requires_grad_(True)
    return conv


def list_source(s, source, conv, with_importance=False):
    """-> (extents, the caller's-list keywords) of one of the three list sources."""
    if source == "scalar":
        return EXTENT, {}
    if source == "rank1":
        return s["rank1"], {}
    idx, rs, d = ops.fixed_radius_search(s["inp_positions"], s["out_positions"], 0.5 * EXTENT)
    kw = dict(user_neighbors_index=idx, user_neighbors_row_splits=rs)
    if with_importance:
        kw["user_neighbors_importance"] = callable_window(d / (0.5 * EXTENT) ** 2)
    return EXTENT, kw


def run(conv, s, extents, **kw):
    kw.setdefault("out_positions", s["out_positions"])
    return conv(s["inp_features"], s["inp_positions"], kw.pop("out_positions"), extents, **kw)


def cases():
    """name -> function(scene) that makes the layer calls of the case."""
    c = {}
    for record in (False, True):
        mode = "record" if record else "infer"
        for source in ("scalar", "rank1", "user"):
            for window in WINDOWS:
                def base(s, record=record, source=source, window=window, cls=ContinuousConv):
                    conv = layer(record, window, cls, **({"record_per_point_extents": True} if record and cls is ContinuousConv else {}))
                    extents, kw = list_source(s, source, conv)
                    run(conv, s, extents, **kw)
                c[f"conv-{mode}-{source}-{window}"] = base
                if not record:
                    c[f"sampling-{source}-{window}"] = lambda s, base=base: base(s, cls=PointSampling)
        for window in ("named", "callable"):
            def hashed(s, record=record, window=window, cls=ContinuousConv):
                table = ops.build_spatial_hash_table(s["inp_positions"], 0.5 * EXTENT)
                run(layer(record, window, cls), s, EXTENT, fixed_radius_search_hash_table=table)
            c[f"conv-{mode}-hash-table-{window}"] = hashed
            if not record:
                c[f"sampling-hash-table-{window}"] = lambda s, hashed=hashed: hashed(s, cls=PointSampling)

        def user_importance(s, record=record, cls=ContinuousConv):
            conv = layer(record, "named", cls)
            extents, kw = list_source(s, "user", conv, with_importance=True)
            run(conv, s, extents, inp_importance=s["importance"], **kw)
        c[f"conv-{mode}-user-importance"] = user_importance
        if not record:
            c["sampling-user-importance"] = lambda s, f=user_importance: f(s, cls=PointSampling)

        def user_importance_empty(s, record=record):
            conv = layer(record)
            extents, kw = list_source(s, "user", conv)
            run(conv, s, extents, user_neighbors_importance=torch.empty(0), **kw)
        c[f"conv-{mode}-user-importance-empty"] = user_importance_empty

        def rank1_user(s, record=record):
            conv = layer(record, record_per_point_extents=True)
            _, kw = list_source(s, "user", conv, with_importance=True)
            run(conv, s, s["rank1"], **kw)
        c[f"conv-{mode}-rank1-user-list"] = rank1_user

        def rank1_unflagged(s, record=record):  # (a refusal while recording)
            run(layer(record), s, s["rank1"])
        c[("refuse-record" if record else "conv-infer") + "-rank1-without-record_per_point_extents"] = rank1_unflagged

        def tensor_extent(s, record=record):
            conv = layer(record)
            run(conv, s, torch.tensor(EXTENT))
            run(conv, s, torch.tensor([EXTENT]))
        c[f"conv-{mode}-extent-as-tensor"] = tensor_extent

        for source in ("scalar", "rank1"):
            for window in ("named", "callable", "none"):
                def batched(s, record=record, source=source, window=window):
                    conv = layer(record, window, record_per_point_extents=True)
                    run(conv, s, list_source(s, source, conv)[0], inp_positions_row_splits=torch.tensor([0, 20, N_INP]),
                        out_positions_row_splits=torch.tensor([0, 16, N_OUT]))
                c[f"conv-{mode}-row-splits-{source}-{window}"] = batched

        for what in ("acc", "extra", "acc+extra"):
            for activation in (None, "relu"):
                def epilogue(s, record=record, what=what, activation=activation, same_points=False, **kw):
                    conv = layer(record, activation=activation, **kw)
                    if "acc" in what:
                        conv.accumulate_into = s["acc_inp" if same_points else "acc"].clone()
                    if "extra" in what:
                        conv.extra_bias = s["extra"]
                    run(conv, s, EXTENT, **({"out_positions": s["inp_positions"]} if same_points else {}))
                c[f"conv-{mode}-{what}-{activation}"] = epilogue
            c[f"conv-{mode}-{what}-dense-centre"] = lambda s, f=epilogue: f(s, activation=None, same_points=True,  # (the centre term: one input per output)
                                                                              use_dense_layer_for_center=True)
            c[f"conv-{mode}-{what}-rank1"] = lambda s, record=record, what=what: _epilogue_rank1(s, record, what)

        def options(s, record=record, same_points=False, **kw):
            conv = layer(record, **kw)
            run(conv, s, EXTENT, **({"out_positions": s["inp_positions"]} if same_points else {}))
        c[f"conv-{mode}-dense-centre"] = lambda s, f=options: f(s, same_points=True, use_dense_layer_for_center=True)
        c[f"conv-{mode}-dense-centre-no-bias"] = lambda s, f=options: f(s, same_points=True, use_dense_layer_for_center=True, use_bias=False)
        c[f"conv-{mode}-no-bias"] = lambda s, f=options: f(s, use_bias=False)
        c[f"conv-{mode}-circular"] = lambda s, f=options: f(s, circular=True)
        c[f"conv-{mode}-symmetric"] = lambda s, f=options: f(s, same_points=True, symmetric=True, kernel_size=[4, 4, 4],
                                                             radius_search_ignore_query_points=True)
        c[f"conv-{mode}-importance"] = lambda s, record=record: run(layer(record), s, EXTENT, inp_importance=s["importance"])
        c[f"conv-{mode}-row-hint"] = lambda s, record=record: _row_hint(s, record)
        if not record:  # (weights are built with requires_grad=False: a first call never records)
            c["conv-infer-lazy-build"] = _lazy_build

        def in_step(s, record=record):
            """Inside a step: the list cache serves the second layer, and only the small operands are kept."""
            a, b, e = layer(record), layer(record, "callable"), layer(record, record_per_point_extents=True)
            ignoring = layer(record, radius_search_ignore_query_points=True)
            for _ in range(2):
                with neighbor_cache():
                    run(a, s, EXTENT)
                    run(b, s, EXTENT)
                    run(a, s, EXTENT)
                    run(e, s, s["rank1"])
                    run(ignoring, s, EXTENT, out_positions=s["inp_positions"])
                    run(layer(False, cls=PointSampling), s, EXTENT)
        c[f"conv-{mode}-in-step"] = in_step
    c.update(refusals())
    return c


def _epilogue_rank1(s, record, what):
    conv = layer(record, record_per_point_extents=True)
    if "acc" in what:
        conv.accumulate_into = s["acc"].clone()
    if "extra" in what:
        conv.extra_bias = s["extra"]
    run(conv, s, s["rank1"])


def _row_hint(s, record):
    conv = layer(record)
    conv.row_length_hint = 2
    run(conv, s, EXTENT)


def _lazy_build(s):
    run(ContinuousConv(COUT, [4, 4, 4], window_function=get_window_func("poly6"), normalize=False, **seeded_weights()), s, EXTENT)


def refusals():
    """Every exception the two layers raise, constructors included (the recorder keeps type and message)."""
    c = {}
    bad_extents = torch.full((2, 2), EXTENT)
    short = torch.full((N_OUT - 1,), EXTENT)
    splits = dict(inp_positions_row_splits=torch.tensor([0, 20, N_INP]), out_positions_row_splits=torch.tensor([0, 16, N_OUT]))
    for record in (False, True):
        mode = "record" if record else "infer"
        c[f"refuse-{mode}-one-row-splits"] = lambda s, r=record: run(layer(r), s, EXTENT, inp_positions_row_splits=splits["inp_positions_row_splits"])
        c[f"refuse-{mode}-row-splits-and-list"] = lambda s, r=record: run(layer(r), s, EXTENT, **splits, **list_source(s, "user", None)[1])
        c[f"refuse-{mode}-row-splits-symmetric"] = lambda s, r=record: run(layer(r, symmetric=True), s, EXTENT, **splits)
        c[f"refuse-{mode}-row-splits-short-rank1"] = lambda s, r=record: run(layer(r), s, short, **splits)
        c[f"refuse-{mode}-row-splits-extents-shape"] = lambda s, r=record: run(layer(r), s, bad_extents, **splits)
        c[f"refuse-{mode}-extents-shape"] = lambda s, r=record: run(layer(r), s, bad_extents)
        c[f"refuse-{mode}-short-rank1"] = lambda s, r=record: run(layer(r, record_per_point_extents=True), s, short)
        c[f"refuse-{mode}-circular-symmetric"] = lambda s, r=record: run(layer(r, circular=True, symmetric=True), s, EXTENT)
        c[f"refuse-{mode}-symmetric-normalize"] = lambda s, r=record: _symmetric_normalize(s, r)
    c["refuse-sampling-extents-shape"] = lambda s: run(layer(False, cls=PointSampling), s, bad_extents)
    c["refuse-sampling-short-rank1"] = lambda s: run(layer(False, cls=PointSampling), s, short)
    return c


def _symmetric_normalize(s, record):
    conv = layer(record, symmetric=True)
    conv.normalize = True
    run(conv, s, EXTENT, out_positions=s["inp_positions"])


CONSTRUCTOR_REFUSALS = {
    "activation": lambda: ContinuousConv(4, [4, 4, 4], activation="gelu"),
    "coordinate_mapping": lambda: ContinuousConv(4, [4, 4, 4], coordinate_mapping="cube"),
    "interpolation": lambda: ContinuousConv(4, [4, 4, 4], interpolation="cubic"),
    "offset": lambda: ContinuousConv(4, [4, 4, 4], offset=[0.0, 0.5, 0.0]),
    "initializer": lambda: ContinuousConv(4, [4, 4, 4], kernel_initializer="he_normal", device="cpu").build(3),
    "scatter-guard": lambda: convolutions._scatter_guard([0, 1]),
}

CASES = cases()


def transcript(name, monkeypatch):
    install_backend(monkeypatch)
    monkeypatch.setattr(convolutions, "_CACHE", convolutions._PerThreadCache())  # (no consumer counts from another case's steps)
    rec = ct.Recorder(monkeypatch)
    try:
        CASES[name](scene())
    except Exception as e:  # (kept with type and message in the layer's own record; here for what the layer never saw)
        rec.records.append({"case_raised": {"type": type(e).__name__, "message": str(e)}})
    return rec.records


@pytest.fixture(scope="module")
def golden():
    if os.environ.get("DMCF_CAPTURE_TRANSCRIPTS") == "1":
        mp = pytest.MonkeyPatch()
        got = {}
        for name in CASES:
            with mp.context() as m:
                got[name] = transcript(name, m)
        for name, make in CONSTRUCTOR_REFUSALS.items():
            with pytest.raises(Exception) as e:
                make()
            got["construct-" + name] = [{"case_raised": {"type": e.type.__name__, "message": str(e.value)}}]
        ct.dump(got, os.path.join(ct.GOLDEN, GOLDEN_FILE))
    return ct.load(GOLDEN_FILE)


def test_the_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(list(CASES) + ["construct-" + k for k in CONSTRUCTOR_REFUSALS])


@pytest.mark.parametrize("name", list(CASES))
def test_transcript_equals_the_recorded_one(name, golden, monkeypatch):
    got = transcript(name, monkeypatch)
    assert ct.first_difference(golden[name], got) is None
    if name.startswith("refuse-"):
        assert "raised" in got[-2] and "case_raised" in got[-1]
    else:
        assert all("raised" not in r and "case_raised" not in r for r in got)


@pytest.mark.parametrize("name", list(CONSTRUCTOR_REFUSALS))
def test_constructor_refusal(name, golden):
    with pytest.raises(Exception) as e:
        CONSTRUCTOR_REFUSALS[name]()
    assert golden["construct-" + name] == ct.digest([{"case_raised": {"type": e.type.__name__, "message": str(e.value)}}])


def test_the_comparison_catches_one_altered_keyword(golden, monkeypatch):
    name = "conv-infer-scalar-named"
    changed = transcript(name, monkeypatch)
    assert ct.first_difference(golden[name], changed) is None
    assert ct.first_difference(golden[name], changed[:-1]) == "3 records != 2"
    options = changed[1]["args"]["geometry"]  # (the stand-in's name for the keywords it does not read)
    assert changed[1]["call"] == "cconv_forward" and options["normalize"] is False
    options["normalize"] = True
    found = ct.first_difference(golden[name], changed)
    assert found.startswith(f"record 1: golden {golden[name][1]!r}, got 'cconv_forward ") and '"normalize": true' in found
    del options["normalize"]
    assert ct.first_difference(golden[name], changed).startswith("record 1:")
    result = changed[2]["result"]  # the bytes of the result
    result["crc"] += 1
    options["normalize"] = False
    assert ct.first_difference(golden[name], changed).startswith("record 2:")
