"""CPU checks of PointNet (dmcf_neighbor_dense_*): symbols, the ctypes mirrors, host-side validation, kernel names, the
model's construction and configuration, the float64 restatement (tests/pointnet_ref.py) against the reference's order and
the adjoint identities, and a whole model step through the CPU oracle against a transliteration of models/pointnet.py.
No device is touched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import pointnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["dmcf_neighbor_dense_forward", "dmcf_neighbor_dense_backward_workspace_bytes", "dmcf_neighbor_dense_backward",
       "dmcf_neighbor_dense_kernel_names"]
EINVAL, EUNSUPPORTED = -1, -4
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_version_and_symbols(hip_lib):
    from dmcf_amd import _lib
    assert hip_lib.dmcf_version() >= 21000
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)


@pytest.mark.parametrize("struct,cls,size", [("dmcf_neighbor_dense_args", "NeighborDenseArgs", 136),
                                             ("dmcf_neighbor_dense_backward_args", "NeighborDenseBackwardArgs", 120)])
def test_structs_mirror_header(struct, cls, size):
    from dmcf_amd import _lib
    C = getattr(_lib, cls)
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    body = text[text.index(f"typedef struct {struct} {{"):text.index(f"}} {struct};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(?:const\s+)?([a-z0-9_]+\*?)\s+(\*?)([a-z_]+);", body, flags=re.M)
    assert [f[2] for f in fields] == [f[0] for f in C._fields_]
    ctypes_of = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for (typ, star, name), (_, ctyp) in zip(fields, C._fields_):
        assert ctyp is (ctypes.c_void_p if (typ.endswith("*") or star) else ctypes_of[typ]), name
    assert C.struct_size.offset == 0
    assert ctypes.sizeof(C) == size


def _fwd(cin=8, cout=16, n_in=10, n_out=10, n_pairs=40, **kw):
    from dmcf_amd._lib import NeighborDenseArgs
    a = NeighborDenseArgs()
    a.struct_size = ctypes.sizeof(NeighborDenseArgs)
    a.flags = 1
    a.x, a.n_in, a.cin, a.cout = FAKE, n_in, cin, cout
    a.kernel = FAKE
    a.neighbors_index, a.neighbors_row_splits = FAKE, FAKE
    a.n_out, a.n_pairs = n_out, n_pairs
    a.out = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd(cin=8, cout=16, n_in=10, n_out=10, **kw):
    from dmcf_amd._lib import NeighborDenseBackwardArgs
    b = NeighborDenseBackwardArgs()
    b.struct_size = ctypes.sizeof(NeighborDenseBackwardArgs)
    b.flags = 1
    b.x, b.n_in, b.cin, b.cout, b.kernel = FAKE, n_in, cin, cout, FAKE
    b.grad_out, b.n_out, b.s, b.count = FAKE, n_out, FAKE, FAKE
    b.inv_index, b.inv_row_splits, b.inv_n_pairs = FAKE, FAKE, 40
    b.grad_x, b.grad_kernel, b.grad_bias = FAKE, FAKE, FAKE
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _names(L, a, b):
    buf = ctypes.create_string_buffer(256)
    rc = L.dmcf_neighbor_dense_kernel_names(None if a is None else ctypes.byref(a), None if b is None else ctypes.byref(b), buf, 256)
    return rc, buf.value.decode()


def test_kernel_names(hip_lib):
    assert _names(hip_lib, _fwd(cin=7, cout=64), None) == (0, "nd_gather_mfma<1>")
    assert _names(hip_lib, _fwd(cin=128, cout=3), None) == (0, "nd_gather_mfma<2>")
    assert _names(hip_lib, _fwd(n_out=0), None) == (0, "")
    assert _names(hip_lib, None, _bwd(cin=128, cout=3)) == (0, "nd_gather_mfma<1>;nd_bwd_weight;nd_bwd_weight_reduce")
    assert _names(hip_lib, None, _bwd(cin=7, cout=128, grad_x=None)) == (0, "nd_bwd_weight;nd_bwd_weight_reduce")
    assert _names(hip_lib, None, _bwd(grad_kernel=None, grad_bias=None))[1] == "nd_gather_mfma<1>"
    assert hip_lib.dmcf_neighbor_dense_backward_workspace_bytes(ctypes.byref(_bwd(cin=7, cout=64, n_out=1000))) == 4 * 8 * 8 * 64  # 8 slabs of 128 rows, [S | c] x G


def _rs(values):
    arr = (ctypes.c_int64 * len(values))(*values)
    return ctypes.cast(arr, ctypes.c_void_p).value, arr


@pytest.mark.parametrize("case", ["short", "cin0", "cout0", "cin_neg", "n_in_neg", "x_null", "index_null", "out_null", "kernel_null",
                                  "splits_null", "record_half", "flags", "splits_not_monotone", "splits_end", "splits_start",
                                  "padded_begin"])
def test_forward_validation(hip_lib, case):
    keep = None
    if case == "short":
        a = _fwd()
        a.struct_size -= 8
    elif case == "cin0":
        a = _fwd(cin=0)
    elif case == "cout0":
        a = _fwd(cout=0)
    elif case == "cin_neg":
        a = _fwd(cin=-3)
    elif case == "n_in_neg":
        a = _fwd(n_in=-1)
    elif case == "x_null":
        a = _fwd(x=None)
    elif case == "index_null":
        a = _fwd(neighbors_index=None)
    elif case == "out_null":
        a = _fwd(out=None)
    elif case == "kernel_null":
        a = _fwd(kernel=None)
    elif case == "splits_null":
        a = _fwd(neighbors_row_splits=None)
    elif case == "record_half":
        a = _fwd(record_s=FAKE)
    elif case == "flags":
        a = _fwd(flags=64)
    else:
        splits = {"splits_not_monotone": [0, 5, 3, 8], "splits_end": [0, 2, 4, 7], "splits_start": [1, 2, 4, 8],
                  "padded_begin": [0, 4, 9]}[case]
        ptr, keep = _rs(splits)
        a = _fwd(n_out=len(splits) - 1, n_pairs=8, host_row_splits=ptr)
        if case == "padded_begin":
            a.n_out = 3
            a.neighbors_row_count = FAKE
    assert hip_lib.dmcf_neighbor_dense_forward(ctypes.byref(a), None) == EINVAL
    assert _names(hip_lib, a, None)[0] == EINVAL
    del keep


def test_forward_validation_accepts_nulls_with_zero_sizes_and_good_splits(hip_lib):
    """Null pointers with zero sizes, and consistent host row splits, pass validation (checked through the kernel-name
    query, which validates exactly as the launch does)."""
    assert _names(hip_lib, _fwd(x=None, n_in=0), None)[0] == 0
    assert _names(hip_lib, _fwd(neighbors_index=None, n_pairs=0), None)[0] == 0
    assert _names(hip_lib, _fwd(out=None, n_out=0), None) == (0, "")
    ptr, keep = _rs([0, 3, 3, 8])
    assert _names(hip_lib, _fwd(n_out=3, n_pairs=8, host_row_splits=ptr), None)[0] == 0
    del keep


def test_unsupported_widths(hip_lib):
    assert hip_lib.dmcf_neighbor_dense_forward(ctypes.byref(_fwd(cin=129)), None) == EUNSUPPORTED
    assert hip_lib.dmcf_neighbor_dense_forward(ctypes.byref(_fwd(cout=200)), None) == EUNSUPPORTED


@pytest.mark.parametrize("case", ["short", "cin0", "cout0", "grad_out_null", "kernel_null", "inv_null", "s_null", "flags", "x_null"])
def test_backward_validation(hip_lib, case):
    b = {"short": lambda: _bwd(), "cin0": lambda: _bwd(cin=0), "cout0": lambda: _bwd(cout=0),
         "grad_out_null": lambda: _bwd(grad_out=None), "kernel_null": lambda: _bwd(kernel=None),
         "inv_null": lambda: _bwd(inv_row_splits=None), "s_null": lambda: _bwd(s=None), "flags": lambda: _bwd(flags=2),
         "x_null": lambda: _bwd(x=None)}[case]()
    if case == "short":
        b.struct_size -= 8
    assert hip_lib.dmcf_neighbor_dense_backward(ctypes.byref(b), None, 0, None) == EINVAL
    assert hip_lib.dmcf_neighbor_dense_backward_workspace_bytes(ctypes.byref(b)) == 0


def test_backward_workspace_too_small(hip_lib):
    b = _bwd(n_out=5000, cin=64, cout=128)
    need = hip_lib.dmcf_neighbor_dense_backward_workspace_bytes(ctypes.byref(b))
    assert need > 0
    assert hip_lib.dmcf_neighbor_dense_backward(ctypes.byref(b), FAKE, need - 4, None) == -2


def test_op_rejects_cpu_tensors(hip_lib):
    import torch
    from dmcf_amd import ops
    from dmcf_amd._lib import DmcfError
    x, W = torch.ones(4, 3), torch.ones(3, 5)
    idx, rs = torch.zeros(4, dtype=torch.int32), torch.tensor([0, 1, 2, 3, 4])
    with pytest.raises(DmcfError):
        ops.neighbor_dense(x, W, None, idx, rs)
    with pytest.raises(DmcfError):
        ops.neighbor_dense(x.requires_grad_(True), W, None, idx, rs)


# ---- configuration and construction ----
def test_pointnet_config_matches_reference_yaml(tmp_path):
    import yaml
    from dmcf_amd.utils.config import Config
    from tools import configs
    with open(os.path.join(GOLDEN, "reference_pointnet_config.json")) as f:
        section = json.load(f)["other/pointnet"]
    path = tmp_path / "pointnet.yml"
    path.write_text(yaml.safe_dump({"model": section}))
    cfg = Config.load_from_file(str(path))
    for k, v in configs.POINTNET2D.items():
        assert cfg.model[k] == v, k
    assert "other/pointnet" not in configs.BY_NAME


def _pointnet_yaml(tmp_path, **model):
    import yaml
    from tools import configs
    with open(os.path.join(GOLDEN, "reference_pointnet_config.json")) as f:
        section = dict(json.load(f)["other/pointnet"], **model)
    cfg = dict(dataset=dict(name="ComplexData"), model=section,
               pipeline=dict(name="Simulator", version="2d", main_log_dir=str(tmp_path / "logs"), output_dir=str(tmp_path / "out"),
                             data_generator=dict(translate=[-0.5, -0.5, 0.0], scale=[1.0, 1.0, 0.0], train=dict(stride=1),
                                                 valid=dict(stride=1, time_end=3), test=dict(stride=1, time_start=0, time_end=3))))
    assert section["name"] == configs.POINTNET2D["name"]
    yml = tmp_path / "pointnet.yml"
    yml.write_text(yaml.safe_dump(cfg))
    return str(yml)


def test_pointnet_builds_and_run_pipeline_builds_it(tmp_path):
    from dmcf_amd import models, run_pipeline
    from tools import configs
    m = models.PointNet(**configs.POINTNET2D)
    assert [d.layer_name for d in m.denses] == ["dense0", "dense1", "dense2", "dense3", "dense4"]
    assert [d.units for d in m.denses] == [64, 128, 128, 128, 3]
    assert "PointNet" in models.__all__
    args, extra = run_pipeline.parse_args(["-c", _pointnet_yaml(tmp_path), "--split", "test", "--dataset_path", GOLDEN])
    pipe = run_pipeline.build(args, extra)
    assert type(pipe.model).__name__ == "PointNet" and pipe.model.layer_channels == [64, 128, 128, 128, 3]
    with pytest.raises(NotImplementedError):
        models.PointNet(out_activation="sigmoid")


def test_load_into_model_takes_a_pointnet_checkpoint():
    """A TensorFlow checkpoint of PointNet holds model/denses/{i}/{kernel,bias} only (PBFNet's input layers are never
    called, so never built): it loads with strict=True; the other models' items are unchanged."""
    from dmcf_amd import models
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs
    m = models.PointNet(**configs.POINTNET2D)
    rng = np.random.default_rng(0)
    widths = [7] + m.layer_channels
    w = {}
    for i in range(5):
        w[f"model/denses/{i}/kernel"] = rng.normal(size=(widths[i], widths[i + 1])).astype(np.float32)
        w[f"model/denses/{i}/bias"] = rng.normal(size=widths[i + 1]).astype(np.float32)
    assert tc.load_into_model(m, w, device="cpu", strict=True) == 5
    for i, d in enumerate(m.denses):
        assert np.array_equal(d.kernel.numpy(), w[f"model/denses/{i}/kernel"]) and np.array_equal(d.bias.numpy(), w[f"model/denses/{i}/bias"])
    cc = models.CConv(**configs.CCONV2D)
    keys = [c[0] for c, _ in tc.model_weight_items(cc)]
    assert "model/fluid_convs" in keys and "model/denses/0" in keys


def test_sharded_simulator_refuses_pointnet():
    from dmcf_amd import models, parallel
    from tools import configs

    class Decomp:
        world = 1

    class Comm:
        world = 1

    with pytest.raises(NotImplementedError):
        parallel.ShardedSimulator(models.PointNet(**configs.POINTNET2D), Comm(), Decomp())


# ---- the float64 restatement ----
def _list(rng, n_out, n_in, max_len=9, oob=0):
    lens = rng.integers(0, max_len, size=n_out)
    rs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, n_in + oob, size=int(rs[-1])).astype(np.int32)
    return idx, rs


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("oob", [0, 5])
def test_restatement_fused_order_equals_reference_order(relu, oob):
    rng = np.random.default_rng(1)
    x = rng.normal(size=(30, 6))
    W, b = rng.normal(size=(6, 5)), rng.normal(size=5)
    idx, rs = _list(rng, 40, 30, oob=oob)
    res = rng.normal(size=(40, 5))
    for r in (None, res):
        a = R.layer_reference_order(x, W, b, idx, rs, relu=relu, residual=r)
        f = R.layer_fused_order(x, W, b, idx, rs, relu=relu, residual=r)
        assert np.allclose(a, f, rtol=1e-12, atol=1e-12)
    # n_in below the rows of x: indices past it read nothing, not even the bias
    a = R.layer_reference_order(x, W, b, idx, rs, n_in=20, relu=relu)
    f = R.layer_fused_order(x, W, b, idx, rs, n_in=20, relu=relu)
    assert np.allclose(a, f, rtol=1e-12, atol=1e-12)
    row = np.repeat(np.arange(40), np.diff(rs))
    only_oob = [r for r in range(40) if rs[r + 1] > rs[r] and np.all(idx[rs[r]:rs[r + 1]] >= 20)]
    for r in only_oob:
        assert np.all(a[r] == 0)
    assert len(row) == len(idx)


@pytest.mark.parametrize("relu", [True, False])
def test_restatement_gradient_through_adjoint_identities(relu):
    """out is linear in W and in b, and positively homogeneous of degree one in x (relu(x) = relu'(x) x), so for any G
    <G, out(x, W, 0)> = <dW, W> = <dx, x> and <G, c b> = <db, b>; plus a central difference in x."""
    rng = np.random.default_rng(2)
    x = rng.normal(size=(25, 4))
    W, b = rng.normal(size=(4, 6)), rng.normal(size=6)
    idx, rs = _list(rng, 30, 25, oob=4)
    G = rng.normal(size=(30, 6))
    dx, dW, db = R.layer_backward(x, W, G, idx, rs, relu=relu)
    y0 = R.layer_reference_order(x, W, None, idx, rs, relu=relu)
    ip = np.sum(G * y0)
    assert np.isclose(ip, np.sum(dW * W), rtol=1e-12)
    assert np.isclose(ip, np.sum(dx * x), rtol=1e-12)
    yb = R.layer_reference_order(x, W, b, idx, rs, relu=relu) - y0
    assert np.isclose(np.sum(G * yb), np.sum(db * b), rtol=1e-12)
    e = np.zeros_like(x)
    e[3, 1] = 1e-6
    fd = (np.sum(G * R.layer_reference_order(x + e, W, b, idx, rs, relu=relu)) -
          np.sum(G * R.layer_reference_order(x - e, W, b, idx, rs, relu=relu))) / 2e-6
    assert np.isclose(fd, dx[3, 1], rtol=1e-6, atol=1e-9)
    # rows past n_in get no gradient
    dx2, _, _ = R.layer_backward(x, W, G, idx, rs, n_in=20, relu=relu)
    assert np.all(dx2[20:] == 0)


# ---- a whole model step through the CPU oracle ----
def _oracle_search(points, radius):
    import oracle as O
    idx, rs, _ = O.fixed_radius_search(np.asarray(points, np.float32), np.asarray(points, np.float32), float(radius))
    return idx, rs


@pytest.mark.parametrize("variant", ["shipped", "no_bnds", "tanh"])
def test_model_step_cpu_against_transliteration(monkeypatch, variant):
    import torch
    import shims
    from dmcf_amd import models, ops
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs, scenes
    shims.install(monkeypatch)

    def neighbor_dense(x, kernel, bias, neighbors_index, neighbors_row_splits, n_in=None, relu=True, residual=None,
                       neighbors_row_count=None, inverted=None):
        y = R.layer_fused_order(x.numpy(), kernel.numpy(), None if bias is None else bias.numpy(), neighbors_index.numpy(),
                                neighbors_row_splits.numpy(), n_in, relu, None if residual is None else residual.numpy())
        return torch.from_numpy(y.astype(np.float32))

    monkeypatch.setattr(ops, "neighbor_dense", neighbor_dense)
    cfg = dict(configs.POINTNET2D)
    if variant == "no_bnds":
        cfg["use_bnds"] = False
    if variant == "tanh":
        cfg["out_activation"] = "tanh"
    model = models.PointNet(**cfg)
    scene = scenes.box_scene(8, h=0.005, dim=2, vel_std=0.05)
    rng = np.random.default_rng(3)
    widths = [7] + model.layer_channels
    weights = []
    w = {}
    for i in range(5):
        k = (rng.normal(size=(widths[i], widths[i + 1])) / np.sqrt(widths[i])).astype(np.float32)
        bb = rng.normal(scale=0.1, size=widths[i + 1]).astype(np.float32)
        w[f"model/denses/{i}/kernel"], w[f"model/denses/{i}/bias"] = k, bb
        weights.append((k, bb))
    tc.load_into_model(model, w, device="cpu")
    data = scenes.model_inputs(scene, grav=[0.0, -9.81, 0.0])
    ref = R.PointNetRef(cfg, weights, _oracle_search)
    pos_ref, vel_ref = ref.step(data)
    tdata = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in data]
    with torch.no_grad():
        pos, vel = model(tdata, training=False)[:2]
    n_fluid = len(scene["pos"])
    assert model.pos_correction.shape == (n_fluid, 3)
    pc = model.pos_correction.numpy()
    assert np.abs(pc - ref.pos_correction).max() <= 1e-4 * np.abs(ref.pos_correction).max() + 1e-12
    assert np.abs(pos.numpy() - pos_ref).max() <= 1e-6 * np.abs(pos_ref).max()
    assert np.array_equal(model.num_fluid_neighbors.numpy(), ref.num_fluid_neighbors)
    if variant != "no_bnds":
        # the layer-0 rule matters here: fluid rows next to the shell have boundary neighbours
        n_all = n_fluid + len(scene["box"])
        assert model.neighbors_row_splits.shape[0] == n_all + 1
        assert int((model.neighbors_index.numpy() >= n_fluid).sum()) > 0
    with pytest.raises(ValueError):
        bad = models.PointNet(**dict(cfg, layer_channels=[7, 3], use_bnds=True, out_activation=None))
        with torch.no_grad():
            bad(tdata, training=False)
